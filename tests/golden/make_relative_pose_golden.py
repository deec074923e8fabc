"""Writes tests/golden/relative_pose_golden.npz: the REFERENCE's RelativePoseFromEssential on the cases of the cheirality stage
(tests/_relative_pose_ref.stage_cases: the lane and row edges, the ratio edge, and the pair without a solution) and its
sfm::robustRelativePose on the pairs of the robust entry at both caller settings, next to the inputs.
Run by hand on the machine that has the reference tree (REFERENCE_SRC, default /root/reference/src): the small driver below - our own
text - is compiled against that tree into a temporary directory outside the repository, run once, and deleted; nothing compiled is kept.

Before the fixture is written the float64 restatement (tests/_relative_pose_ref.py) is held against the compiled reference: the
decisions (ok, the sorted counts, the selected list) must be equal on every pair whose margins are above the guard, at most 5 % of
the pairs may fall below it, and the spread of pose and points between the two is recorded - 1 000 x that spread is the tolerance of
the device tests (tests/_relative_pose_cases.py carries it with the measured spread beside it).
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _relative_pose_ref as rref  # noqa: E402

GOLD_PATH = os.path.join(ROOT, "tests", "golden", "relative_pose_golden.npz")
SRC = os.environ.get("REFERENCE_SRC", "/root/reference/src")
GUARD = 1e-9   # margins are relative quantities of order 1e-1 .. 1; rounding moves them by 1e-15: six orders of room on either side

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "openMVG/cameras/Camera_Pinhole.hpp"
#include "openMVG/multiview/essential.hpp"
#include "openMVG/multiview/motion_from_essential.hpp"
#include "openMVG/multiview/triangulation.hpp"
#include "openMVG/sfm/pipelines/sfm_robust_model_estimation.hpp"
using namespace openMVG;
static void put(FILE* out, const void* p, size_t bytes) { fwrite(p, 1, bytes, out); }
static void put_pose(FILE* out, const geometry::Pose3& pose) {
  const Mat3 R = pose.rotation(); const Vec3 t = pose.translation(), C = pose.center();
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { const double v = R(r, c); put(out, &v, 8); }
  for (int r = 0; r < 3; ++r) { const double v = t(r); put(out, &v, 8); }
  for (int r = 0; r < 3; ++r) { const double v = C(r); put(out, &v, 8); }
}
static int stage(FILE* in, FILE* out) {
  int n_cases = 0;
  if (fread(&n_cases, 4, 1, in) != 1) return 1;
  for (int c = 0; c < n_cases; ++c) {
    int head[3];   // n, list length, method
    double ratio, e[9];
    if (fread(head, 4, 3, in) != 3 || fread(&ratio, 8, 1, in) != 1 || fread(e, 8, 9, in) != 9) return 1;
    const int n = head[0], m = head[1];
    std::vector<double> b(6 * (size_t)n);
    std::vector<uint32_t> use(m);
    if (n && fread(b.data(), 8, b.size(), in) != b.size()) return 1;
    if (m && fread(use.data(), 4, m, in) != (size_t)m) return 1;
    Mat3X x1(3, n), x2(3, n);
    for (int i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { x1(k, i) = b[3 * i + k]; x2(k, i) = b[3 * n + 3 * i + k]; }
    Mat3 E;
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) E(r, k) = e[3 * r + k];
    geometry::Pose3 pose;
    std::vector<uint32_t> selected;
    std::vector<Vec3> points;
    const int ok = RelativePoseFromEssential(x1, x2, E, use, &pose, &selected, &points, ratio, static_cast<ETriangulationMethod>(head[2])) ? 1 : 0;
    // the accumulator is local to that function: the same count again, through the same two functions
    std::vector<geometry::Pose3> poses;
    MotionFromEssential(E, &poses);
    uint32_t counts[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
      for (const uint32_t i : use) {
        Vec3 X;
        if (Triangulate2View(Mat3::Identity(), Vec3::Zero(), x1.col(i), poses[k].rotation(), poses[k].translation(), x2.col(i), X, static_cast<ETriangulationMethod>(head[2])))
          ++counts[k];
      }
    const int best = *std::max_element(counts, counts + 4) ? 1 : 0;   // lists and pose are exported iff some count is above zero
    const int k = best ? (int)selected.size() : 0;
    put(out, &ok, 4); put(out, counts, 16); put(out, &k, 4);
    put_pose(out, best ? pose : geometry::Pose3());
    if (k) put(out, selected.data(), 4 * (size_t)k);
    for (int i = 0; i < k; ++i) for (int a = 0; a < 3; ++a) { const double v = points[i](a); put(out, &v, 8); }
  }
  return 0;
}
static int robust(FILE* in, FILE* out) {
  int n_pairs = 0;
  if (fread(&n_pairs, 4, 1, in) != 1) return 1;
  for (int p = 0; p < n_pairs; ++p) {
    int head[4];   // n, width, height, iterations
    double par[4];   // focal, ppx, ppy, initial_residual_tolerance
    if (fread(head, 4, 4, in) != 4 || fread(par, 8, 4, in) != 4) return 1;
    const int n = head[0];
    std::vector<double> x(4 * (size_t)n);
    if (fread(x.data(), 8, x.size(), in) != x.size()) return 1;
    Mat x1(2, n), x2(2, n);
    for (int i = 0; i < n; ++i) { x1(0, i) = x[2 * i]; x1(1, i) = x[2 * i + 1]; x2(0, i) = x[2 * n + 2 * i]; x2(1, i) = x[2 * n + 2 * i + 1]; }
    const cameras::Pinhole_Intrinsic cam(head[1], head[2], par[0], par[1], par[2]);
    sfm::RelativePose_Info info;
    info.initial_residual_tolerance = par[3];
    const std::pair<size_t, size_t> size(head[1], head[2]);
    const int ok = sfm::robustRelativePose(&cam, &cam, x1, x2, info, size, size, (size_t)head[3]) ? 1 : 0;
    const int k = (int)info.vec_inliers.size();
    put(out, &ok, 4); put(out, &k, 4); put(out, &info.found_residual_precision, 8);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { const double v = info.essential_matrix(r, c); put(out, &v, 8); }
    put_pose(out, ok ? info.relativePose : geometry::Pose3());
    if (k) put(out, info.vec_inliers.data(), 4 * (size_t)k);
  }
  return 0;
}
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  const int rc = strcmp(argv[1], "stage") == 0 ? stage(in, out) : robust(in, out);
  fclose(out);
  return rc;
}
"""


def compile_driver(tmp):
    open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
    mv, num = os.path.join(SRC, "openMVG", "multiview"), os.path.join(SRC, "openMVG", "numeric")
    srcs = [os.path.join(mv, f) for f in ("motion_from_essential.cpp", "essential.cpp", "triangulation.cpp", "projection.cpp", "conditioning.cpp",
                                          "solver_essential_five_point.cpp", "solver_essential_eight_point.cpp", "solver_essential_three_point.cpp", "solver_essential_kernel.cpp",
                                          "solver_fundamental_kernel.cpp")]
    srcs += [os.path.join(num, "numeric.cpp"), os.path.join(num, "nullspace.cpp"), os.path.join(SRC, "openMVG", "sfm", "pipelines", "sfm_robust_model_estimation.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-DEIGEN_MPL2_ONLY", "-I" + SRC, "-I" + os.path.join(SRC, "third_party", "eigen"), "-I" + os.path.join(SRC, "third_party"),
                    "-I" + os.path.join(SRC, "dependencies", "cereal", "include"), os.path.join(tmp, "driver.cpp")] + srcs + ["-o", os.path.join(tmp, "driver")], check=True)
    return os.path.join(tmp, "driver")


def run_reference(cases, xI, xJ, start):
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        a, b = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(a, "wb") as f:
            f.write(np.int32(len(cases)).tobytes())
            for c in cases:
                n = len(c["bI"])
                use = np.arange(n, dtype=np.uint32) if c["use"] is None else np.asarray(c["use"], np.uint32)
                f.write(np.array([n, len(use), c["method"]], np.int32).tobytes() + np.float64(c["ratio"]).tobytes() + np.ascontiguousarray(c["E"], np.float64).tobytes() +
                        np.ascontiguousarray(c["bI"], np.float64).tobytes() + np.ascontiguousarray(c["bJ"], np.float64).tobytes() + use.tobytes())
        subprocess.run([exe, "stage", a, b], check=True)
        raw = open(b, "rb").read()
        stage, at = [], 0
        for _ in cases:
            ok, c0, c1, c2, c3, k = struct.unpack_from("i4Ii", raw, at)
            pose = np.frombuffer(raw, np.float64, 15, at + 24).copy()
            sel = np.frombuffer(raw, np.uint32, k, at + 144).copy()
            pts = np.frombuffer(raw, np.float64, 3 * k, at + 144 + 4 * k).reshape(-1, 3).copy()
            at += 144 + 28 * k
            stage.append(dict(ok=bool(ok), counts=(c0, c1, c2, c3), pose=pose, selected=sel, points=pts))
        assert at == len(raw)
        robust = []
        for tol, it in rref.ROBUST_SETTINGS:
            with open(a, "wb") as f:
                f.write(np.int32(len(start) - 1).tobytes())
                for p in range(len(start) - 1):
                    lo, hi = int(start[p]), int(start[p + 1])
                    f.write(np.array([hi - lo, rref.IMAGE_WH[0], rref.IMAGE_WH[1], it], np.int32).tobytes() + np.array([rref.FOCAL, 500.0, 500.0, tol]).tobytes() +
                            np.ascontiguousarray(xI[lo:hi]).tobytes() + np.ascontiguousarray(xJ[lo:hi]).tobytes())
            subprocess.run([exe, "robust", a, b], check=True)
            raw = open(b, "rb").read()
            at, rows = 0, []
            for p in range(len(start) - 1):
                ok, k = struct.unpack_from("ii", raw, at)
                prec, = struct.unpack_from("d", raw, at + 8)
                E = np.frombuffer(raw, np.float64, 9, at + 16).copy()
                pose = np.frombuffer(raw, np.float64, 15, at + 88).copy()
                inl = np.frombuffer(raw, np.uint32, k, at + 208).copy()
                at += 208 + 4 * k
                rows.append(dict(ok=bool(ok), precision=prec, E=E, pose=pose, inliers=np.sort(inl)))
            assert at == len(raw)
            robust.append(rows)
    return stage, robust


if __name__ == "__main__":
    cases = rref.stage_cases()
    E0, bI0, bJ0 = rref.no_solution_pair()
    cases += [dict(key=("none", m, 3, 0), method=m, ratio=0.7, E=E0, bI=bI0, bJ=bJ0, use=None) for m in range(4)]
    xI, xJ, start = rref.robust_cases()
    stage, robust = run_reference(cases, xI, xJ, start)

    # ---- the restatement against the compiled reference ----
    below, spread_pose, spread_points = [], 0.0, 0.0
    for c, r in zip(cases, stage):
        own = rref.relative_pose_from_essential(c["bI"], c["bJ"], c["E"], c["use"], c["ratio"], c["method"])
        # (the ratio's own margin is recorded, not guarded: second / best is one division of two integers - the same double wherever the
        # counts are the same - and the ratio edge sits at a margin of exactly 0 on purpose)
        if own.point_margin < GUARD:
            below.append(c["key"])
            continue
        assert own.ok == r["ok"] and sorted(own.cheirality) == sorted(r["counts"]), (c["key"], own.ok, r["ok"], own.cheirality, r["counts"])
        if own.ok:
            assert np.array_equal(own.selected, r["selected"]), c["key"]
            spread_pose = max(spread_pose, float(np.abs(np.concatenate([own.R.ravel(), own.t, own.center]) - r["pose"]).max()))
            if len(own.points):
                spread_points = max(spread_points, float((np.abs(own.points - r["points"]).max(axis=1) / np.maximum(1.0, np.abs(r["points"]).max(axis=1))).max()))
        if c["key"][0] == "ratio":   # the construction itself: the counts are (m, k, 0, 0), the verdict as the issue of the ratio edge states
            m, k = c["key"][2], c["key"][3]
            assert sorted(r["counts"]) == sorted((m, k, 0, 0)), (c["key"], r["counts"])
            assert r["ok"] == ((m, k) in ((10, 6), (17, 3))), c["key"]
        if c["key"][0] == "none":
            assert not r["ok"] and max(r["counts"]) == 0, (c["key"], r["counts"])
    assert len(below) <= 0.05 * len(cases), f"more than 5 % of the cases below the guard: {below}"
    print("stage:", len(cases), "cases, below the guard", below, "spread of pose", spread_pose, "of points (relative)", spread_points)
    print("tolerances (x 1000): pose", 1000 * spread_pose, "points", 1000 * spread_points)
    for (tol, it), rows in zip(rref.ROBUST_SETTINGS, robust):
        print("robust", tol, it, "ok", sum(r["ok"] for r in rows), "of", len(rows), "inliers", [len(r["inliers"]) for r in rows])
        assert not rows[-1]["ok"] and len(rows[-1]["inliers"]) < 13

    uniq = list({id(c["bI"]): c for c in cases}.values())
    cat = lambda rows, k, dt: (np.concatenate([np.asarray(r[k], dt).reshape(-1) for r in rows]) if rows else np.zeros(0, dt))   # noqa: E731
    np.savez_compressed(
        GOLD_PATH,
        stage_key=np.array([[{"edge": 0, "ratio": 1, "none": 2}[c["key"][0]], *c["key"][1:]] for c in cases], np.int32),
        stage_method=np.array([c["method"] for c in cases], np.int32), stage_ratio=np.array([c["ratio"] for c in cases]),
        # every input once: the four methods share their geometry (stage_input[i] = the record of case i)
        stage_input=np.array([[id(d["bI"]) for d in uniq].index(id(c["bI"])) for c in cases], np.int64),
        stage_E=np.array([c["E"] for c in uniq]), stage_n=np.array([len(c["bI"]) for c in uniq], np.int64),
        stage_bI=np.concatenate([c["bI"].reshape(-1, 3) for c in uniq]), stage_bJ=np.concatenate([c["bJ"].reshape(-1, 3) for c in uniq]),
        stage_use_n=np.array([-1 if c["use"] is None else len(c["use"]) for c in cases], np.int64),
        stage_use=cat([c for c in cases if c["use"] is not None], "use", np.uint32),
        stage_ok=np.array([r["ok"] for r in stage]), stage_counts=np.array([r["counts"] for r in stage], np.uint32),
        stage_pose=np.array([r["pose"] for r in stage]), stage_n_selected=np.array([len(r["selected"]) for r in stage], np.int64),
        stage_selected=cat(stage, "selected", np.uint32), stage_points=cat(stage, "points", np.float64).reshape(-1, 3),
        spread=np.array([spread_pose, spread_points]), guard=np.float64(GUARD),
        robust_xI=xI, robust_xJ=xJ, robust_start=start, robust_settings=np.array(rref.ROBUST_SETTINGS),
        robust_ok=np.array([[r["ok"] for r in rows] for rows in robust]), robust_precision=np.array([[r["precision"] for r in rows] for rows in robust]),
        robust_E=np.array([[r["E"] for r in rows] for rows in robust]), robust_pose=np.array([[r["pose"] for r in rows] for rows in robust]),
        robust_n_inliers=np.array([[len(r["inliers"]) for r in rows] for rows in robust], np.int64),
        robust_inliers=np.concatenate([cat(rows, "inliers", np.uint32) for rows in robust]))
    print(os.path.getsize(GOLD_PATH), "bytes")
