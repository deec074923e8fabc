"""Writes tests/golden/resection_dlt_golden.npz: the REFERENCE's resection without intrinsics, next to the outputs of the float64
restatement (tests/_resection_dlt_ref.py) on the same inputs and the spread between the two:
  (a) SixPointResectionSolver::Solve on seeded six-point samples (400 general ones with 0.5 px noise - twelve equations for eleven degrees
      of freedom: the null vector is a least-squares one -, the three depth outcomes, near-coplanar sextuples around the ratio gate), and
      the ratio of singular values that gates it (NullspaceRatio on the reference's own design matrix);
  (b) ACRANSAC through the reference's own ACKernelAdaptorResection<SixPointResectionSolver, SquaredPixelReprojectionError,
      UnnormalizerResection, Mat34> on the parity grid of tests/_resection_dlt_cases.py (36 runs).
Run by hand on the machine that has the reference tree (REFERENCE_SRC, default /root/reference/src): the small driver below - our own
text - is compiled against that tree into a temporary directory outside the repository, run once, and deleted; nothing compiled is kept.
The adaptor and ACRANSAC are header-only; solver_resection_kernel.cpp, projection.cpp, conditioning.cpp and numeric.cpp are linked.

Before the fixture is written the restatement is held against the compiled reference: a run of the grid whose inlier lists differ must
have a decision margin below the guard (1 000 x the NFA spread of the equal runs), and at most 5 % of the 36 runs (one) may be such.
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _resection_dlt_ref as dref  # noqa: E402
from tests import _resection_ref as ref  # noqa: E402

GOLD_PATH = os.path.join(ROOT, "tests", "golden", "resection_dlt_golden.npz")
SRC = os.environ.get("REFERENCE_SRC", "/root/reference/src")
N_SAMPLES, SEED = 400, 20261020
PARITY_OUTLIERS, PARITY_S, PARITY_ITERATIONS = (0.0, 0.3, 0.6), (1, 2, 3), (9, 10, 40, 4096)

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "openMVG/multiview/solver_resection_kernel.hpp"
#include "openMVG/multiview/solver_resection_metrics.hpp"
#include "openMVG/robust_estimation/robust_estimator_ACRansac.hpp"
#include "openMVG/robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp"
namespace openMVG { namespace resection { namespace kernel {   // defined in solver_resection_kernel.cpp, not declared in its header
void translate(const Mat3X& X, const Vec3& vecTranslation, Mat3X* XPoints);
double NullspaceRatio(const Eigen::Ref<const Mat>& A, Eigen::Ref<Vec> nullspace);
void BuildActionMatrix(Eigen::Ref<Mat> A, const Mat& pt2D, const Mat& XPoints);
}}}
using namespace openMVG;
static int solver(FILE* in, FILE* out) {
  int n = 0;
  if (fread(&n, sizeof(int), 1, in) != 1) return 1;
  std::vector<double> x(12 * n), X(18 * n);
  if (fread(x.data(), sizeof(double), x.size(), in) != x.size() || fread(X.data(), sizeof(double), X.size(), in) != X.size()) return 1;
  for (int i = 0; i < n; ++i) {
    Mat xm(2, 6), Xm(3, 6);
    for (int v = 0; v < 6; ++v) {
      for (int c = 0; c < 2; ++c) xm(c, v) = x[12 * i + 2 * v + c];
      for (int c = 0; c < 3; ++c) Xm(c, v) = X[18 * i + 3 * v + c];
    }
    std::vector<Mat34> models;
    resection::kernel::SixPointResectionSolver::Solve(xm, Xm, &models, true);
    Mat3X Xt;
    resection::kernel::translate(Xm, -Xm.col(0), &Xt);
    Mat A = Mat::Zero(12, 12);
    resection::kernel::BuildActionMatrix(A, xm, Xt);
    Vec p(12);
    const double ratio = resection::kernel::NullspaceRatio(A, p);
    const int count = (int)models.size();
    fwrite(&count, sizeof(int), 1, out);
    fwrite(&ratio, sizeof(double), 1, out);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) { const double v = count ? models[0](r, c) : 0.0; fwrite(&v, sizeof(double), 1, out); }
  }
  return 0;
}
static int loop(FILE* in, FILE* out) {
  int n_runs = 0;
  if (fread(&n_runs, sizeof(int), 1, in) != 1) return 1;
  for (int r = 0; r < n_runs; ++r) {
    int head[4];   // n, width, height, max_iteration
    if (fread(head, sizeof(int), 4, in) != 4) return 1;
    const int n = head[0];
    std::vector<double> buf(5 * n);
    if (fread(buf.data(), sizeof(double), buf.size(), in) != buf.size()) return 1;
    Mat x2d(2, n), X(3, n);
    for (int i = 0; i < n; ++i) {
      x2d(0, i) = buf[2 * i]; x2d(1, i) = buf[2 * i + 1];
      for (int c = 0; c < 3; ++c) X(c, i) = buf[2 * n + 3 * i + c];
    }
    using KernelType = robust::ACKernelAdaptorResection<resection::kernel::SixPointResectionSolver, resection::SquaredPixelReprojectionError,
                                                        robust::UnnormalizerResection, Mat34>;
    KernelType kernel(x2d, head[1], head[2], X);
    std::vector<uint32_t> inliers;
    Mat34 P = Mat34::Zero();
    const std::pair<double, double> res = robust::ACRANSAC(kernel, inliers, (unsigned)head[3], &P, std::numeric_limits<double>::infinity(), false);
    const int k = (int)inliers.size();
    fwrite(&k, sizeof(int), 1, out);
    fwrite(&res.first, sizeof(double), 1, out); fwrite(&res.second, sizeof(double), 1, out);
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 4; ++c) { const double v = P(a, c); fwrite(&v, sizeof(double), 1, out); }
    if (k) fwrite(inliers.data(), sizeof(uint32_t), k, out);
  }
  return 0;
}
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  const int rc = strcmp(argv[1], "solver") == 0 ? solver(in, out) : loop(in, out);
  fclose(out);
  return rc;
}
"""


def compile_driver(tmp):
    open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
    mv = os.path.join(SRC, "openMVG", "multiview")
    subprocess.run(["g++", "-O2", "-std=c++17", "-DEIGEN_MPL2_ONLY", "-I" + SRC, "-I" + os.path.join(SRC, "third_party", "eigen"), "-I" + os.path.join(SRC, "third_party"),
                    os.path.join(tmp, "driver.cpp"), os.path.join(mv, "solver_resection_kernel.cpp"), os.path.join(mv, "projection.cpp"),
                    os.path.join(mv, "conditioning.cpp"), os.path.join(SRC, "openMVG", "numeric", "numeric.cpp"), "-o", os.path.join(tmp, "driver")], check=True)
    return os.path.join(tmp, "driver")


def run_reference(x, X, runs):
    """-> (count, ratio, P) of the solver on the samples; [(inliers, error_max, min_nfa, P)] of ACRANSAC on runs = [(problem, max_iteration)]"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        a, b = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(a, "wb") as f:
            f.write(np.int32(len(x)).tobytes() + np.ascontiguousarray(x).tobytes() + np.ascontiguousarray(X).tobytes())
        subprocess.run([exe, "solver", a, b], check=True)
        rec = np.dtype([("count", np.int32), ("ratio", np.float64), ("P", np.float64, (3, 4))], align=False)
        got = np.fromfile(b, np.uint8).view(rec)
        solver = got["count"].copy(), got["ratio"].copy(), got["P"].copy()
        with open(a, "wb") as f:
            f.write(np.int32(len(runs)).tobytes())
            for pr, it in runs:
                f.write(np.array([len(pr["x2d"]), dref.IMAGE_WH[0], dref.IMAGE_WH[1], it], np.int32).tobytes() + np.ascontiguousarray(pr["x2d"]).tobytes() +
                        np.ascontiguousarray(pr["X3d"]).tobytes())
        subprocess.run([exe, "loop", a, b], check=True)
        raw = open(b, "rb").read()
    out, at = [], 0
    for _ in runs:
        k, = struct.unpack_from("i", raw, at)
        err, nfa = struct.unpack_from("2d", raw, at + 4)
        P = np.frombuffer(raw, np.float64, 12, at + 20).reshape(3, 4).copy()
        inl = np.frombuffer(raw, np.uint32, k, at + 116).copy()
        at += 116 + 4 * k
        out.append((inl, err, nfa, P))
    return solver, out


def rel_P(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


if __name__ == "__main__":
    x, X, group = dref.solver_samples(N_SAMPLES, seed=SEED)
    grid = [(o, s, it) for it in PARITY_ITERATIONS for s in PARITY_S for o in PARITY_OUTLIERS]
    (ref_count, ref_ratio, ref_P), loop = run_reference(x, X, [(dref.parity_problem(o, s), it) for o, s, it in grid])

    # ---- the solver ----
    own_count, own_ratio, own_P = np.zeros(len(x), np.int32), np.zeros(len(x)), np.zeros((len(x), 3, 4))
    gate_margin = np.zeros(len(x))
    branches = set()
    for i in range(len(x)):
        mg = ref.Margin()
        models, own_ratio[i] = dref.six_point(x[i], X[i], mg, branches)
        own_count[i], gate_margin[i] = len(models), mg.value
        if models:
            own_P[i] = models[0]
    both = (ref_count == 1) & (own_count == 1)
    solver_spread = np.array([max(rel_P(own_P[i], ref_P[i]) for i in np.flatnonzero(both)), float(np.abs(own_ratio / ref_ratio - 1.0).max())])

    # ---- the loop ----
    own = [dref.localize(dref.parity_problem(o, s)["x2d"], dref.parity_problem(o, s)["X3d"], max_iteration=it) for o, s, it in grid]
    loop_same = np.array([np.array_equal(inl, w.inliers) for (inl, _, _, _), w in zip(loop, own)])
    nfa_spread = err_spread = P_spread = 0.0
    for (inl, err, nfa, P), w, same in zip(loop, own, loop_same):
        if same and np.isfinite(nfa):   # (a run without any model: minNFA = infinity in both)
            nfa_spread = max(nfa_spread, abs(nfa - w.min_nfa) / max(abs(nfa), 1.0))
            if len(inl):
                err_spread = max(err_spread, abs(err - w.error_max) / abs(err))
            if w.P is not None:
                P_spread = max(P_spread, rel_P(w.P, P))
    loop_spread = np.array([nfa_spread, err_spread, P_spread])
    guard = 1000.0 * nfa_spread
    print("solver: models", np.bincount(ref_count), "per group", {int(g): int(ref_count[group == g].sum()) for g in np.unique(group)}, "spread (|dP| relative, ratio relative)",
          solver_spread, "branches", sorted(branches))
    print("loop: equal inlier lists in", int(loop_same.sum()), "of", len(grid), "runs; spreads (relative NFA, relative threshold, relative |dP|)", loop_spread, "guard", guard)
    # the restatement against the compiled reference, inside the cap
    decided = gate_margin >= guard
    assert np.array_equal(ref_count[decided], own_count[decided]), "the restatement returns another number of models than the reference on a decided sample"
    left_out = [g for g, same, w in zip(grid, loop_same, own) if not same and w.margin < guard]
    wrong = [g for g, same, w in zip(grid, loop_same, own) if not same and w.margin >= guard]
    assert not wrong, f"the restatement parts from the reference with a margin above the guard: {wrong}"
    assert len(left_out) <= 0.05 * len(grid), f"more than 5 % of the grid left out: {left_out}"
    np.savez_compressed(
        GOLD_PATH, x_norm=x, X=X, group=group, ref_count=ref_count, ref_ratio=ref_ratio, ref_P=ref_P, own_count=own_count, own_ratio=own_ratio, own_P=own_P,
        solver_spread=solver_spread, loop_grid=np.array(grid), loop_same=loop_same, loop_min_nfa=np.array([r[2] for r in loop]),
        loop_error_max=np.array([r[1] for r in loop]), loop_P=np.array([r[3] for r in loop]), loop_n_inliers=np.array([len(r[0]) for r in loop]),
        loop_inliers=np.concatenate([r[0] for r in loop]), own_min_nfa=np.array([w.min_nfa for w in own]), own_error_max=np.array([w.error_max for w in own]),
        own_loop_P=np.array([w.P if w.P is not None else np.zeros((3, 4)) for w in own]),
        own_n_iterations=np.array([w.n_iterations for w in own]), loop_spread=loop_spread)
    print("left out", left_out, os.path.getsize(GOLD_PATH), "bytes")
