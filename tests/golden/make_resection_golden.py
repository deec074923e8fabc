"""Writes tests/golden/resection_golden.npz: the REFERENCE's P3PSolver_Ding::Solve and P3PSolver_Nordberg::Solve on seeded noise-free
samples, next to the outputs of the float64 restatement (tests/_resection_ref.py) on the same samples and the spread between the two.
Run by hand on the machine that has the reference tree (REFERENCE_SRC, default /root/reference/src): the small driver below - our own
text - is compiled against that tree into a temporary directory outside the repository, run once, and deleted; nothing compiled is kept.

The loop is recorded through the reference's header-only ACRANSAC template (exhaustive NFA, loop, pool sampler, logcombi tables) over the
reference's Ding solver, on the parity grid of tests/_resection_cases.py: inlier list, threshold, minNFA and model per run, and the
spread against the restatement over the runs in which both return the same list. SfM_Localizer::Localize itself is not linked: its kernel
adaptor is defined in SfM_Localizer.cpp beside RefinePose, which needs Ceres and the sfm library; the loop driver's adaptor (bearings
ready-made, plain pinhole / spherical projection, N1) is our own text.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _resection_ref as ref  # noqa: E402

GOLD_PATH = os.path.join(ROOT, "tests", "golden", "resection_golden.npz")
SRC = os.environ.get("REFERENCE_SRC", "/root/reference/src")
N_SAMPLES, SEED = 400, 20261020

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "openMVG/multiview/solver_resection_p3p_ding.hpp"
#include "openMVG/multiview/solver_resection_p3p_nordberg.hpp"
using namespace openMVG;
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int n = 0;
  if (!in || !out || fread(&n, sizeof(int), 1, in) != 1) return 1;
  std::vector<double> b(9 * n), X(9 * n);
  if (fread(b.data(), sizeof(double), b.size(), in) != b.size() || fread(X.data(), sizeof(double), X.size(), in) != X.size()) return 1;
  for (int solver = 0; solver < 2; ++solver)
    for (int i = 0; i < n; ++i) {
      Mat bm(3, 3), Xm(3, 3);
      for (int v = 0; v < 3; ++v)
        for (int c = 0; c < 3; ++c) { bm(c, v) = b[9 * i + 3 * v + c]; Xm(c, v) = X[9 * i + 3 * v + c]; }
      std::vector<Mat34> models;
      if (solver == 0) euclidean_resection::P3PSolver_Ding::Solve(bm, Xm, &models);
      else euclidean_resection::P3PSolver_Nordberg::Solve(bm, Xm, &models);
      const int count = (int)models.size();
      fwrite(&count, sizeof(int), 1, out);
      for (int m = 0; m < 4; ++m)
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 4; ++c) { const double v = m < count ? models[m](r, c) : 0.0; fwrite(&v, sizeof(double), 1, out); }
    }
  fclose(out);
  return 0;
}
"""


# The loop: robust_estimator_ACRansac.hpp is header-only, so the reference's ACRANSAC template (exhaustive NFA, loop, pool sampler, logcombi
# tables) is instantiated here over the reference's P3P solver with a kernel adaptor of OUR OWN text - ACKernelAdaptorResection_Intrinsics
# lives in SfM_Localizer.cpp beside RefinePose and does not link without Ceres. The adaptor takes the bearings ready-made and projects
# with the plain pinhole / spherical formulas.
LOOP_DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include "openMVG/multiview/solver_resection_p3p_ding.hpp"
#include "openMVG/numeric/extract_columns.hpp"
#include "openMVG/robust_estimation/robust_estimator_ACRansac.hpp"
using namespace openMVG;
struct Adaptor {
  using Model = Mat34;
  enum { MINIMUM_SAMPLES = 3 };
  enum { MAX_MODELS = 4 };
  Mat x2d, X, bear; int model; double intr[8]; double n1;
  void Fit(const std::vector<uint32_t>& samples, std::vector<Model>* models) const {
    euclidean_resection::P3PSolver_Ding::Solve(ExtractColumns(bear, samples), ExtractColumns(X, samples), models);
  }
  void Errors(const Model& M, std::vector<double>& e) const {
    e.resize(x2d.cols());
    for (Mat::Index i = 0; i < x2d.cols(); ++i) {
      const Vec3 p = M.block<3, 3>(0, 0) * X.col(i) + M.col(3);
      double u, v;
      if (model == 7) {
        const double w = intr[0], h = intr[1], k = std::max(w, h) / (2.0 * M_PI);
        u = std::atan2(p(0), p(2)) * k + w / 2.0; v = -std::atan2(-p(1), std::hypot(p(0), p(2))) * k + h / 2.0;
      } else { u = intr[1] + intr[0] * (p(0) / p(2)); v = intr[2] + intr[0] * (p(1) / p(2)); }
      const double rx = (x2d(0, i) - u) * n1, ry = (x2d(1, i) - v) * n1;
      e[i] = rx * rx + ry * ry;
    }
  }
  size_t NumSamples() const { return x2d.cols(); }
  void Unnormalize(Model*) const {}
  double logalpha0() const { return log10(M_PI); }
  double multError() const { return 1.0; }
  Mat3 normalizer1() const { return Mat3::Identity(); }
  Mat3 normalizer2() const { Mat3 N = Mat3::Identity(); N(0, 0) = N(1, 1) = n1; return N; }
  double unormalizeError(double val) const { return sqrt(val) / n1; }
};
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int n_runs = 0;
  if (!in || !out || fread(&n_runs, sizeof(int), 1, in) != 1) return 1;
  for (int r = 0; r < n_runs; ++r) {
    int head[3];   // n, model, max_iteration
    Adaptor A;
    if (fread(head, sizeof(int), 3, in) != 3 || fread(A.intr, sizeof(double), 8, in) != 8 || fread(&A.n1, sizeof(double), 1, in) != 1) return 1;
    const int n = head[0];
    A.model = head[1];
    std::vector<double> buf(8 * n);
    if (fread(buf.data(), sizeof(double), buf.size(), in) != buf.size()) return 1;
    A.x2d.resize(2, n); A.X.resize(3, n); A.bear.resize(3, n);
    for (int i = 0; i < n; ++i) {
      A.x2d(0, i) = buf[2 * i]; A.x2d(1, i) = buf[2 * i + 1];
      for (int c = 0; c < 3; ++c) { A.X(c, i) = buf[2 * n + 3 * i + c]; A.bear(c, i) = buf[5 * n + 3 * i + c]; }
    }
    std::vector<uint32_t> inliers;
    Mat34 P = Mat34::Zero();
    const std::pair<double, double> res = robust::ACRANSAC(A, inliers, (unsigned)head[2], &P, std::numeric_limits<double>::infinity(), false);
    const int k = (int)inliers.size();
    fwrite(&k, sizeof(int), 1, out);
    fwrite(&res.first, sizeof(double), 1, out); fwrite(&res.second, sizeof(double), 1, out);
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 4; ++c) { const double v = P(a, c); fwrite(&v, sizeof(double), 1, out); }
    if (k) fwrite(inliers.data(), sizeof(uint32_t), k, out);
  }
  fclose(out);
  return 0;
}
"""


def compile_driver(tmp, text, name, extra=()):
    open(os.path.join(tmp, name + ".cpp"), "w").write(text)
    mv = os.path.join(SRC, "openMVG", "multiview")
    subprocess.run(["g++", "-O2", "-std=c++17", "-DEIGEN_MPL2_ONLY", "-I" + SRC, "-I" + os.path.join(SRC, "third_party", "eigen"), "-I" + os.path.join(SRC, "third_party"),
                    os.path.join(tmp, name + ".cpp"), os.path.join(mv, "solver_resection_p3p_ding.cpp"),
                    os.path.join(mv, "solver_resection_p3p_nordberg.cpp"), os.path.join(mv, "projection.cpp"),
                    os.path.join(SRC, "openMVG", "numeric", "numeric.cpp"), *extra, "-o", os.path.join(tmp, name)], check=True)
    return os.path.join(tmp, name)


def run_reference_loop(runs):
    """runs: [(problem dict, max_iteration)] -> [(inliers, error_max, min_nfa, P)] of the reference's ACRANSAC"""
    import struct
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp, LOOP_DRIVER, "loop_driver")
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.int32(len(runs)).tobytes())
            for pr, it in runs:
                n = len(pr["x2d"])
                f.write(np.array([n, pr["model"], it], np.int32).tobytes() + np.asarray(pr["intr"], np.float64).tobytes() +
                        np.float64(ref.n1_of(pr["model"], pr["intr"])).tobytes() + np.ascontiguousarray(pr["x2d"]).tobytes() +
                        np.ascontiguousarray(pr["X3d"]).tobytes() + np.ascontiguousarray(ref.bearings(pr["model"], pr["intr"], pr["x2d"])).tobytes())
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, at = [], 0
    for _ in runs:
        k, = struct.unpack_from("i", raw, at)
        err, nfa = struct.unpack_from("2d", raw, at + 4)
        P = np.frombuffer(raw, np.float64, 12, at + 20).reshape(3, 4).copy()
        inl = np.frombuffer(raw, np.uint32, k, at + 116).copy()
        at += 116 + 4 * k
        out.append((inl, err, nfa, P))
    return out


def run_reference(B, X):
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
        mv = os.path.join(SRC, "openMVG", "multiview")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DEIGEN_MPL2_ONLY", "-I" + SRC, "-I" + os.path.join(SRC, "third_party", "eigen"),
                        os.path.join(tmp, "driver.cpp"), os.path.join(mv, "solver_resection_p3p_ding.cpp"),
                        os.path.join(mv, "solver_resection_p3p_nordberg.cpp"), os.path.join(mv, "projection.cpp"),
                        os.path.join(SRC, "openMVG", "numeric", "numeric.cpp"), "-o", os.path.join(tmp, "driver")], check=True)
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.int32(len(B)).tobytes() + np.ascontiguousarray(B).tobytes() + np.ascontiguousarray(X).tobytes())
        subprocess.run([os.path.join(tmp, "driver"), os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
        raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
    rec = np.dtype([("count", np.int32), ("Rt", np.float64, (4, 3, 4))])
    got = raw.view(rec).reshape(2, len(B))
    return got["count"].copy(), got["Rt"].copy()


def restatement(B, X):
    count = np.zeros((2, len(B)), np.int32)
    Rt = np.zeros((2, len(B), 4, 3, 4))
    for s, solver in enumerate((ref.DING, ref.NORDBERG)):
        for i in range(len(B)):
            models = ref.SOLVERS[solver](B[i], X[i])
            count[s, i] = len(models)
            for m, M in enumerate(models):
                Rt[s, i, m] = M
    return count, Rt


if __name__ == "__main__":
    B, X, R, t = ref.p3p_samples(N_SAMPLES, seed=SEED)
    ref_count, ref_Rt = run_reference(B, X)
    own_count, own_Rt = restatement(B, X)
    assert np.array_equal(ref_count, own_count), "the restatement returns another number of models than the reference"
    spread = np.abs(ref_Rt - own_Rt).max(axis=(1, 2, 3, 4))   # per solver
    truth = np.concatenate([R, t[:, :, None]], 2)
    ref_error = np.array([[min((np.abs(ref_Rt[s, i, m] - truth[i]).max() for m in range(ref_count[s, i])), default=np.inf) for i in range(len(B))]
                          for s in range(2)])
    # the loop on the parity grid of tests/_resection_cases.py: the reference's ACRANSAC against the restatement left to itself. The two
    # part where the order of a sample's own noise-level residuals differs (tests/_resection_ref.py); the spreads are taken over the
    # runs whose inlier lists are equal, order included - there both ran the same samples.
    from tests import _resection_cases as cases  # noqa: E402
    grid = [(m, o, it) for it in cases.PARITY_ITERATIONS for m in cases.PARITY_MODELS for o in cases.PARITY_OUTLIERS]
    loop = run_reference_loop([(cases.parity_problem(m, o), it) for m, o, it in grid])
    loop_same, nfa_spread, err_spread, P_spread = [], 0.0, 0.0, 0.0
    for (m, o, it), (inl, err, nfa, P) in zip(grid, loop):
        pr = cases.parity_problem(m, o)
        own = ref.localize(m, pr["intr"], pr["x2d"], pr["X3d"], max_iteration=it)
        same = np.array_equal(inl, own.inliers)
        loop_same.append(same)
        if same:
            nfa_spread = max(nfa_spread, abs(nfa - own.min_nfa) / max(abs(nfa), 1.0))
            if len(inl):
                err_spread = max(err_spread, abs(err - own.error_max) / abs(err))
            if own.P is not None:
                P_spread = max(P_spread, float(np.abs(P - own.P).max()))
    loop_arrays = dict(loop_grid=np.array(grid), loop_same=np.array(loop_same), loop_min_nfa=np.array([r[2] for r in loop]),
                       loop_error_max=np.array([r[1] for r in loop]), loop_P=np.array([r[3] for r in loop]),
                       loop_n_inliers=np.array([len(r[0]) for r in loop]), loop_inliers=np.concatenate([r[0] for r in loop]),
                       loop_spread=np.array([nfa_spread, err_spread, P_spread]))
    print("loop: restatement and reference return the same inlier list (order included) in", int(np.sum(loop_same)), "of", len(grid),
          "runs; spreads there (relative NFA, relative threshold, |dP|):", loop_arrays["loop_spread"])
    np.savez_compressed(GOLD_PATH, bearings=B, X=X, R=R, t=t, ref_count=ref_count, ref_Rt=ref_Rt, own_Rt=own_Rt, solver_spread=spread,
                        ref_error=ref_error, **loop_arrays)
    print("samples", len(B), "models per sample", np.bincount(ref_count.ravel()), "spread (ding, nordberg)", spread,
          "largest error of the reference's best model", ref_error.max(axis=1), os.path.getsize(GOLD_PATH), "bytes")
