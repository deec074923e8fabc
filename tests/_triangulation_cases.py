"""What the emulation and the GPU tests of mvgx_triangulate_tracks share: the comparison with the restatement and its tolerances."""
import numpy as np

from openmvg_amd import triangulation
from tests import _triangulation_ref as ref

# Largest |dX| between the restatement and the compiled reference (tests/test_triangulation_ref_cpu.py prints them; DESIGN.md,
# "Triangulation"), per solver. The device may differ from the restatement by 1000 x that: three orders for its summation grouping,
# fused multiply-adds, f64 division and sqrt sequences and its Jacobi eigen-solver - about 2e-11 on coordinates of order 1.
SPREAD = {"closed": 3.6e-15, "dlt": 1.6e-14, "nview": 2.4e-15}
MIN_MARGIN = 1e-6   # guard on the INPUTS: no decision of the restatement, no gap between two hypothesis errors closer than this


def solver_of(mode, n, method, k):
    """which solver produces the point of a track of n observations"""
    if mode == "blind":
        return "closed" if n == 2 else "nview"
    views = n if (n == k) else k   # the all-observations case triangulates the whole track (n == min_required == k)
    if views > 2:
        return "nview"
    return "dlt" if method == ref.DLT else "closed"


def x_tolerance(sc, mode, method, k):
    n = np.diff(np.asarray(sc["track_start"]).astype(np.int64))
    return np.array([1000.0 * SPREAD[solver_of(mode, int(v), method, k)] for v in n])


_CACHE = {}


def reference(name, sc, **kw):
    """the restatement's result for a named case (the name stands for the scene), computed once per process"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = ref.triangulate(*ref.args_of(sc), obs_defined=sc.get("obs_defined"), **kw)
    return _CACHE[key]


def run_device(sc, mode="robust", method=ref.IDW_MIDPOINT, min_required_inliers=3, min_sample_index=3, max_reprojection_error=4.0):
    return triangulation.triangulate_tracks(*ref.args_of(sc), mode=mode, method=method, max_reprojection_error=max_reprojection_error,
                                            min_required_inliers=min_required_inliers, min_sample_index=min_sample_index,
                                            obs_defined=sc.get("obs_defined"))


def compare(name, sc, mode="robust", method=ref.IDW_MIDPOINT, min_required_inliers=3, min_sample_index=3, guard=True):
    """Runs the library (whatever _capi routes to) and the restatement on the scene: decisions equal, every track's X within the
    tolerance of its solver. Returns (device result, restatement, largest |dX|)."""
    kw = dict(mode=mode, method=method, min_required_inliers=min_required_inliers, min_sample_index=min_sample_index)
    want = reference(name, sc, **kw)
    print(f"{name} {kw}: restatement margin {want.margin:.3g}, gap {want.gap:.3g}, kept {int(want.ok.sum())}/{len(want.ok)}")
    if guard:
        assert want.margin >= MIN_MARGIN and want.gap >= MIN_MARGIN, "the inputs sit on a decision boundary: choose another seed"
    X, ok, inl, stats = run_device(sc, **kw)
    dev = float(np.abs(X - want.X).max()) if len(X) else 0.0
    print(f"{name}: largest |dX| device vs restatement {dev:.3g}")
    assert np.array_equal(ok, want.ok)
    assert np.array_equal(inl[: len(want.inl)], want.inl)
    assert stats.n_hypotheses == want.n_hypotheses
    assert stats.n_tracks == len(ok) and stats.n_kept == int(want.ok.sum()) and stats.n_inlier_obs == int(want.inl.sum())
    assert np.all(X[~want.ok] == 0.0)
    tol = x_tolerance(sc, mode, method, min_sample_index)
    assert np.all(np.abs(X - want.X).max(axis=1) <= tol), (np.abs(X - want.X).max(axis=1) / tol).max()
    return (X, ok, inl, stats), want, dev


def mixed_lengths(n_tracks, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, n_tracks)
