"""CPU: the float64 restatement of the reference's triangulation (tests/_triangulation_ref.py) against what it restates - the
oracle's camera code, std::mt19937 and, where oracle/_ref/libref_geofilter.so exists, the compiled reference's Triangulate2View."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import _oracle
from tests import _triangulation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_geofilter.so")
# bool openMVG::Triangulate2View(Mat3 const&, Vec3 const&, Vec3 const&, Mat3 const&, Vec3 const&, Vec3 const&, Vec3&, ETriangulationMethod)
TRIANGULATE2VIEW = ("_ZN7openMVG16Triangulate2ViewERKN5Eigen6MatrixIdLi3ELi3ELi0ELi3ELi3EEERKNS1_IdLi3ELi1ELi0ELi3ELi1EEES7_S4_S7_S7_RS5_"
                    "NS_20ETriangulationMethodE")


def test_generator_and_sample_tables():
    bg = ref._mt19937()
    assert int(bg.random_raw()) == 3499211612   # the first output of std::mt19937(5489)
    for k, n in ((2, 2), (2, 5), (3, 3), (3, 7), (3, 70)):
        tab = ref.sample_table(k, n)
        assert len(tab) == 2 * n
        for s in tab:
            assert len(s) == k and list(s) == sorted(set(s)) and 0 <= s[0] and s[-1] < n
    # the bounded draw, by hand: (raw * n) >> 32 where no rejection applies
    bg = ref._mt19937()
    raw = [int(bg.random_raw()) for _ in range(3)]
    assert ref.sample_table(3, 1000)[0] == tuple(sorted((r * 1000) >> 32 for r in raw))


@pytest.mark.parametrize("model", ref.MODELS)
def test_residuals_match_the_oracle(built_lib, model):
    rng = np.random.default_rng(100 + model)
    sc = ref.scene(8, [6] * 12, model=model, seed=3 + model)
    worst = 0.0
    for o in range(len(sc["obs_pose"])):
        pose = sc["poses"][sc["obs_pose"][o]]
        X = sc["points"][o // 6] + 0.01 * rng.standard_normal(3)
        xy = sc["obs_xy"][o]
        want = _oracle.port_ba_eval_obs(model, sc["intrinsics"][0], pose, X, xy)[0]
        p = ref.to_camera(ref.rotation(pose[:3]), pose[3:6], X)
        got = ref.residual(model, [float(v) for v in sc["intrinsics"][0]], p, (float(xy[0]), float(xy[1])))
        worst = max(worst, abs(got[0] - want[0]), abs(got[1] - want[1]))
    print(f"model {model}: largest residual difference {worst:.3g} px")
    assert worst < 1e-9   # pixels of order 1e3, rotations formed by two routes: a few thousand ulp at most


@pytest.mark.parametrize("model", ref.MODELS)
def test_undistorted_bearings_match_the_oracle(built_lib, model):
    """Two-observation tracks: the angle between R^T b_ud of the restatement's bearings is what the oracle's track-angle filter returns."""
    sc = ref.scene(8, [2] * 40, model=model, seed=11 + model)
    flat = dict(poses=sc["poses"], intrinsics=sc["intrinsics"], intr_model=sc["intr_model"], points=sc["points"], obs_pose=sc["obs_pose"],
                obs_intr=sc["obs_intr"], obs_point=np.repeat(np.arange(40, dtype=np.uint32), 2), obs_xy=sc["obs_xy"])
    want = _oracle.port_ba_track_angles(flat)
    intr = [float(v) for v in sc["intrinsics"][0]]
    worst = 0.0
    for t in range(40):
        rays = []
        for o in (2 * t, 2 * t + 1):
            R = ref.rotation(sc["poses"][sc["obs_pose"][o]][:3])
            b = ref.bearing(model, intr, sc["obs_xy"][o], True)
            rays.append(ref._normalized(tuple(R[0][j] * b[0] + R[1][j] * b[1] + R[2][j] * b[2] for j in range(3))))
        dt = min(max(ref._dot(rays[0], rays[1]), -1.0 + 1e-8), 1.0 - 1e-8)
        worst = max(worst, abs(math.degrees(math.acos(dt)) - want[t]))
    print(f"model {model}: largest angle difference {worst:.3g} deg")
    assert worst < 1e-9   # angles of tens of degrees: acos amplifies a rounding error of the dot product by 1 / sin(angle) < 10


def test_raw_bearing_skips_the_undistortion():
    for model in ref.MODELS:
        intr = [float(v) for v in ref.model_intrinsics(model, np.random.default_rng(0))]
        ud, raw = ref.bearing(model, intr, (812.0, 301.0), True), ref.bearing(model, intr, (812.0, 301.0), False)
        assert abs(math.sqrt(ref._dot(raw, raw)) - 1.0) < 1e-15
        same = model in (ref.PINHOLE, ref.SPHERICAL)
        assert (ud == raw) == same


def _camera_pairs(n_pairs, seed=2024):
    """two cameras of the ring scene family and the (noisy) pinhole bearings of one point in them"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_pairs:
        sc = ref.scene(8, [2] * 250, model=ref.PINHOLE, seed=int(rng.integers(1 << 30)))
        intr = [float(v) for v in sc["intrinsics"][0]]
        for t in range(250):
            v = []
            for o in (2 * t, 2 * t + 1):
                pose = sc["poses"][sc["obs_pose"][o]]
                v.append((ref.rotation(pose[:3]), tuple(float(x) for x in pose[3:6]), ref.bearing(ref.PINHOLE, intr, sc["obs_xy"][o], True)))
            out.append(v)
    return out[:n_pairs]


def compiled_two_view():
    """openMVG::Triangulate2View of the compiled reference as f(method, R0, t0, b0, R1, t1, b1) -> (ok, X)"""
    fn = getattr(C.CDLL(REF_SO), TRIANGULATE2VIEW)
    fn.restype = C.c_bool
    fn.argtypes = [C.c_void_p] * 7 + [C.c_ubyte]
    col = lambda R: np.ascontiguousarray(np.asarray(R, np.float64).T).reshape(-1)   # Mat3: 9 doubles, column-major
    vec = lambda v: np.ascontiguousarray(v, np.float64)

    def call(method, R0, t0, b0, R1, t1, b1):
        a = [col(R0), vec(t0), vec(b0), col(R1), vec(t1), vec(b1), np.zeros(3)]
        ok = bool(fn(*[x.ctypes.data for x in a], method))
        return ok, a[6]
    return call


needs_compiled_reference = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libref_geofilter.so (the compiled reference) is not built")


@needs_compiled_reference
def test_two_view_solvers_match_the_compiled_reference():
    """All four methods on 2 000 camera pairs: equal decisions; the largest |dX| per method is printed (recorded in DESIGN.md)."""
    fn = compiled_two_view()
    pairs = _camera_pairs(2000)
    for method in (ref.DLT, ref.L1_ANGULAR, ref.LINF_ANGULAR, ref.IDW_MIDPOINT):
        worst, mismatches = 0.0, 0
        for (R0, t0, b0), (R1, t1, b1) in pairs:
            want_ok, want_X = fn(method, R0, t0, b0, R1, t1, b1)
            ok, X = ref.two_view(method, R0, t0, b0, R1, t1, b1)
            mismatches += ok != want_ok
            worst = max(worst, float(np.abs(np.asarray(X) - want_X).max()))
        print(f"method {method}: largest |dX| restatement vs compiled reference {worst:.3g}, decision mismatches {mismatches}")
        assert mismatches == 0
        assert worst < 1e-12   # coordinates of order 1: the two are the same formulas, a few ulp apart (see DESIGN.md for the figures)


@needs_compiled_reference
@pytest.mark.parametrize("family", range(5))
def test_two_view_solvers_against_50_digits(family):
    """The compiled Triangulate2View on the two-view families of tests/golden/triangulation_truth.npz (scenes away from the origin, small
    parallax) against the 50-digit points: its error within 10 x the restatement's and the restatement's within 10 x its own - the two are
    one yardstick on the hard geometry too, where they are no longer equal to 1e-12."""
    from tests import _triangulation_accuracy_cases as acc
    from tests import _triangulation_truth as truth
    gen, fx, fn = acc.generator(), acc.fixture(), compiled_two_view()
    key = f"f{family}_v2_"
    for solver in gen.SOLVERS_OF[2]:
        got = []
        for poses, xy in zip(fx[key + "poses"], fx[key + "xy"]):
            ok, X = gen.compiled_reference(fn, solver, poses, xy)
            assert ok
            got.append(X)
        hi, lo = fx[key + solver + "_hi"], fx[key + solver + "_lo"]
        e_compiled = float(truth.error(np.array(got), hi, lo).max())
        e_ref = float(truth.error(fx[key + solver + "_ref"], hi, lo).max())
        print(f"family {tuple(fx['families'][family])} {solver}: compiled reference vs 50 digits {e_compiled:.3g}, restatement {e_ref:.3g}")
        assert e_compiled <= 10.0 * e_ref and e_ref <= 10.0 * e_compiled
