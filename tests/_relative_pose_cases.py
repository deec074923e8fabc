"""The cases of the relative-pose tests, shared by tests/test_relative_pose_emu_cpu.py (the device code under the HIP emulation) and
tests/test_relative_pose_gpu.py (-m gpu): mvgx_relative_pose_from_essential and mvgx_relative_pose_robust against the compiled
reference's outputs (tests/golden/relative_pose_golden.npz, written by tests/golden/make_relative_pose_golden.py) and the float64
restatement (tests/_relative_pose_ref.py).

Tolerances. The generator of the fixture measured the spread between restatement and compiled reference on the cases of the cheirality
stage - two float64 evaluations of the same formulas that differ in the SVD behind them and in the order of a few sums:
    pose (R, t, centre; absolute, entries of order 1)      SPREAD_POSE
    points (relative to max(1, |X|))                       SPREAD_POINTS
The device is a third such evaluation (one-sided Jacobi, fused multiply-adds); its tolerance is that spread x 1 000, the project's
usual margin between "differs by rounding" and "differs".
The robust entry adds one term: its E is the a-contrario model of the device, which agrees with the reference's to rounding of the
five-point solver, not bit for bit (the filter's own tests bound the difference of the normalised models by 1e-6 on pairs with equal
inlier sets, tests/_geofilter_cases.py). The singular vectors of a matrix move by at most |dE| / gap (Wedin), the gap between the
second and third singular value of an essential matrix of unit Frobenius norm is 1 / sqrt(2), and R is a product of both sets of
vectors: |dR|, |dt| <= 2 sqrt(2) |dE| < 10 x the largest entry of dE. So there the pose tolerance is TOL_POSE + 10 |dE|, with |dE|
measured on the pair and held below the filter's 1e-6.
"""
import ctypes as C
import functools
import math
import os

import numpy as np

from openmvg_amd import _capi, geofilter
from openmvg_amd import relative_pose as rp
from tests import _geofilter_cases
from tests import _relative_pose_ref as rref

# measured by tests/golden/make_relative_pose_golden.py on the 64 cases of the stage (it prints them; the fixture carries them as "spread")
SPREAD_POSE, SPREAD_POINTS = 1.5543122344752192e-15, 7.241614802682905e-14
TOL_POSE, TOL_POINTS = 1000.0 * SPREAD_POSE, 1000.0 * SPREAD_POINTS   # 1.6e-12, 7.2e-11
GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relative_pose_golden.npz")
KIND = {0: "edge", 1: "ratio", 2: "none"}


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD_PATH))


@functools.lru_cache(maxsize=None)
def stage_cases():
    """{key: case} - the inputs of the fixture with the reference's outputs (ref_*) beside them"""
    g = gold()
    out, at_use, at_sel = {}, 0, 0
    first = np.concatenate([[0], np.cumsum(g["stage_n"])])   # (the four methods share their inputs: stage_input names the record)
    for i, row in enumerate(g["stage_key"]):
        rec, un, k = int(g["stage_input"][i]), int(g["stage_use_n"][i]), int(g["stage_n_selected"][i])
        lo, hi = int(first[rec]), int(first[rec + 1])
        c = dict(method=int(g["stage_method"][i]), ratio=float(g["stage_ratio"][i]), E=g["stage_E"][rec], bI=g["stage_bI"][lo:hi], bJ=g["stage_bJ"][lo:hi],
                 use=None if un < 0 else g["stage_use"][at_use:at_use + un], ref_ok=bool(g["stage_ok"][i]), ref_counts=tuple(int(v) for v in g["stage_counts"][i]),
                 ref_pose=g["stage_pose"][i], ref_selected=g["stage_selected"][at_sel:at_sel + k], ref_points=g["stage_points"][at_sel:at_sel + k])
        out[(KIND[int(row[0])],) + tuple(int(v) for v in row[1:])] = c
        at_use += max(un, 0); at_sel += k
    return out


def tolerances():
    """(pose, points): 1 000 x the spread the generator measured between restatement and compiled reference"""
    assert tuple(float(v) for v in gold()["spread"]) == (SPREAD_POSE, SPREAD_POINTS), "the fixture was regenerated: carry its spread over"
    return TOL_POSE, TOL_POINTS


# ---- the C entry as it is, on outputs filled with sentinels: what a call must not touch stays recognisable ----
SENTINEL_U32, SENTINEL_F64 = 0xDEADBEEF, -77.25


def call_from_essential(cases, explicit_lists, opt=None, **broken):
    """One call on the batch `cases`. explicit_lists: every pair passes its list (its own `use`, or 0 .. n - 1), else use_index = NULL
    (every `use` must be None). broken: arguments replaced before the call (the argument-error cases). -> (rc, dict of the outputs)"""
    n_pairs = len(cases)
    start = np.concatenate([[0], np.cumsum([len(c["bI"]) for c in cases])]).astype(np.uint64)
    bI = np.ascontiguousarray(np.concatenate([c["bI"].reshape(-1, 3) for c in cases] + [np.zeros((1, 3))]))
    bJ = np.ascontiguousarray(np.concatenate([c["bJ"].reshape(-1, 3) for c in cases] + [np.zeros((1, 3))]))
    E = np.ascontiguousarray(np.array([c["E"] for c in cases], np.float64).reshape(-1, 9))
    use_start = use_index = None
    n_list = int(start[-1])
    if explicit_lists:
        lists = [np.arange(len(c["bI"]), dtype=np.uint32) if c["use"] is None else np.asarray(c["use"], np.uint32) for c in cases]
        use_start = np.concatenate([[0], np.cumsum([len(u) for u in lists])]).astype(np.uint64)
        use_index = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.uint32)]))
        n_list = int(use_start[-1])
    else:
        assert all(c["use"] is None for c in cases)
    if opt is None:
        opt = rp.default_options(method=cases[0]["method"], positive_depth_ratio=cases[0]["ratio"])
    elif opt is False:   # a NULL options pointer
        opt = None
    res = np.zeros(n_pairs + 1, rp._RESULT)
    res.view(np.uint8)[:] = 0xAB
    out = dict(res=res, sel_start=np.full(n_pairs + 1, 2 ** 64 - 1, np.uint64), sel=np.full(n_list + 8, SENTINEL_U32, np.uint32), X=np.full((n_list + 8, 3), SENTINEL_F64))
    args = dict(n_pairs=n_pairs, start=start, bI=bI, bJ=bJ, E=E, use_start=use_start, use_index=use_index, opt=opt, res=out["res"], sel_start=out["sel_start"],
                sel=out["sel"], X=out["X"])
    args.update(broken)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a   # noqa: E731
    rc = _capi.lib().mvgx_relative_pose_from_essential(-1, args["n_pairs"], P(args["start"]), P(args["bI"]), P(args["bJ"]), P(args["E"]), P(args["use_start"]),
                                                       P(args["use_index"]), C.byref(args["opt"]) if args["opt"] is not None else None, P(args["res"]),
                                                       P(args["sel_start"]), P(args["sel"]), P(args["X"]), None)
    out["n_list"] = n_list
    return rc, out


def untouched(out, n_results=0, n_listed=0):
    """the sentinels behind what a call may write (everything, for a refused call)"""
    return (bool((out["res"].view(np.uint8)[n_results * rp._RESULT.itemsize:] == 0xAB).all()) and bool((out["sel"][n_listed:] == SENTINEL_U32).all()) and
            bool((out["X"][n_listed:] == SENTINEL_F64).all()) and (n_results > 0 or bool((out["sel_start"] == 2 ** 64 - 1).all())))


def check_against_reference(c, row, selected, points, key):
    """one pair of a call against the fixture's RelativePoseFromEssential and the restatement"""
    tol_pose, tol_points = tolerances()
    own = rref.relative_pose_from_essential(c["bI"], c["bJ"], c["E"], c["use"], c["ratio"], c["method"])
    counts = tuple(int(v) for v in row["cheirality"])
    assert bool(row["ok"]) == c["ref_ok"] == own.ok, (key, row["ok"], c["ref_ok"], own.ok)
    assert sorted(counts) == sorted(c["ref_counts"]) == sorted(own.cheirality), (key, counts, c["ref_counts"], own.cheirality)
    if not c["ref_ok"]:
        assert int(row["n_selected"]) == 0 and len(selected) == 0 and not row["pose"].any(), key
        return
    assert int(row["n_selected"]) == max(counts) == len(selected), (key, row["n_selected"], counts)   # the device-side invariant of the two passes
    assert np.array_equal(selected, c["ref_selected"]) and np.array_equal(selected, own.selected), key
    d_pose = float(np.abs(row["pose"][[0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 7, 11, 12, 13, 14]] - c["ref_pose"]).max())
    assert d_pose <= tol_pose, (key, d_pose, tol_pose)
    if len(points):
        d_pts = float((np.abs(points - c["ref_points"]).max(axis=1) / np.maximum(1.0, np.abs(c["ref_points"]).max(axis=1))).max())
        assert d_pts <= tol_points, (key, d_pts, tol_points)


def run_batch(keys, explicit_lists):
    cs = stage_cases()
    cases = [cs[k] for k in keys]
    rc, out = call_from_essential(cases, explicit_lists)
    assert rc == _capi.MVGX_OK, _capi.lib().mvgx_last_error()
    ss = out["sel_start"]
    assert int(ss[0]) == 0 and (np.diff(ss.astype(np.int64)) >= 0).all()
    for p, (k, c) in enumerate(zip(keys, cases)):
        lo, hi = int(ss[p]), int(ss[p + 1])
        assert hi - lo == int(out["res"][p]["n_selected"]), k
        assert np.array_equal(out["res"][p]["E"], np.asarray(c["E"]).reshape(9)) and out["res"][p]["found_precision"] == 0.0 and out["res"][p]["n_acransac_inliers"] == 0
        check_against_reference(c, out["res"][p], out["sel"][lo:hi], out["X"][lo:hi], k)
    assert untouched(out, len(cases), int(ss[-1])), "the call wrote behind its lists or results"
    return out


# ---- 1. lane and row edges ----
def check_edges(method, explicit_lists):
    """the nine lengths in one batch: with lists (those of 63 and 129 correspondences vote with a shuffled subset), and with use_index = NULL"""
    keys = [("edge", method, n, 1 if explicit_lists and n in rref.SUBSET_OF else 0) for n in rref.EDGE_LENS]
    out = run_batch(keys, explicit_lists)
    # the empty pair, and the pairs beside it
    assert out["res"][0]["ok"] == 0 and not out["res"][0]["pose"].any() and tuple(out["res"][0]["cheirality"]) == (0, 0, 0, 0)
    assert int(out["sel_start"][1]) == 0 and out["res"][1]["ok"] == 1
    # the same pairs in another order, the empty one in the middle: every pair's result is its own
    order = [3, 0, 8, 1]
    again = run_batch([keys[i] for i in order], explicit_lists)
    for q, i in enumerate(order):
        assert all(again["res"][q][f].tobytes() == out["res"][i][f].tobytes() for f in rp._RESULT.names), (method, i)   # (field by field: the struct ends in padding)


# ---- 2. the ratio edge ----
def check_ratio(method):
    keys = [("ratio", method, m, k) for m, k in rref.RATIO_CASES]
    out = run_batch(keys, False)
    assert [int(r["ok"]) for r in out["res"][:4]] == [0, 0, 1, 1]
    for p, (m, k) in enumerate(rref.RATIO_CASES):
        assert sorted(int(v) for v in out["res"][p]["cheirality"]) == sorted((m, k, 0, 0))


# ---- 3. no solution ----
def check_no_solution(method):
    out = run_batch([("none", method, 3, 0), ("edge", method, 17, 0)], False)
    assert out["res"][0]["ok"] == 0 and not out["res"][0]["pose"].any() and out["res"][0]["n_selected"] == 0 and out["res"][1]["ok"] == 1


# ---- 4. argument errors ----
def check_arguments():
    cs = stage_cases()
    cases = [cs[("edge", 3, 17, 0)], cs[("edge", 3, 63, 1)]]
    bad_opt = lambda **kw: rp.default_options(**kw)   # noqa: E731
    for explicit, broken in [(True, dict(start=None)), (True, dict(bI=None)), (True, dict(bJ=None)), (True, dict(E=None)), (True, dict(res=None)), (True, dict(sel_start=None)),
                             (True, dict(sel=None)), (True, dict(X=None)), (True, dict(opt=False)), (True, dict(use_start=None)),
                             (True, dict(start=np.array([0, 17, 5], np.uint64))), (True, dict(use_start=np.array([0, 17, 9], np.uint64))),
                             (True, dict(opt=bad_opt(positive_depth_ratio=0.0))), (True, dict(opt=bad_opt(positive_depth_ratio=1.5))),
                             (True, dict(opt=bad_opt(positive_depth_ratio=math.nan))), (True, dict(opt=bad_opt(method=4))), (True, dict(opt=bad_opt(method=-1)))]:
        rc, out = call_from_essential(cases, explicit, **broken)
        assert rc == _capi.MVGX_ERR_ARG, (broken.keys(), rc)
        assert all(untouched(dict(out, **{k: v})) for k, v in [("res", out["res"])]), broken.keys()
    # an index outside its pair: the first pair has 17 correspondences
    lists = np.concatenate([np.arange(17), cases[1]["use"], [0]]).astype(np.uint32)
    lists[5] = 17
    rc, out = call_from_essential(cases, True, use_index=lists)
    assert rc == _capi.MVGX_ERR_ARG and untouched(out)
    # ratio 1 is inside (0, 1]
    rc, out = call_from_essential(cases, True, opt=rp.default_options(positive_depth_ratio=1.0))
    assert rc == _capi.MVGX_OK and out["res"][0]["ok"] == 1
    # the robust entry
    xI, xJ, start, wh, K = robust_inputs(range(2))
    for kw, code in [(dict(tolerance=math.inf), _capi.MVGX_ERR_UNSUPPORTED), (dict(tolerance=0.0), _capi.MVGX_ERR_ARG), (dict(tolerance=-1.0), _capi.MVGX_ERR_ARG),
                     (dict(tolerance=math.nan), _capi.MVGX_ERR_ARG), (dict(ratio=0.0), _capi.MVGX_ERR_ARG), (dict(ratio=1.01), _capi.MVGX_ERR_ARG),
                     (dict(method=7), _capi.MVGX_ERR_ARG), (dict(max_iterations=0), _capi.MVGX_ERR_ARG)]:
        try:
            rp.robust(xI, xJ, start, wh, K, **kw)
        except _capi.MvgxError as e:
            assert e.code == code, (kw, e.code)
        else:
            raise AssertionError(f"robust accepted {kw}")
    try:
        rp.robust_angular(np.zeros((30, 3)), np.zeros((30, 3)), [0, 30], tolerance_deg=math.inf)
    except _capi.MvgxError as e:
        assert e.code == _capi.MVGX_ERR_UNSUPPORTED
    else:
        raise AssertionError("robust_angular accepted an unbounded tolerance")


# ---- 5. the robust entry, pinhole ----
def robust_inputs(pairs):
    """the fixture's pairs `pairs` as one batch -> xI, xJ, start, image_wh, K"""
    g = gold()
    s = g["robust_start"].astype(np.int64)
    pairs = list(pairs)
    xI = np.concatenate([g["robust_xI"][s[p]:s[p + 1]] for p in pairs])
    xJ = np.concatenate([g["robust_xJ"][s[p]:s[p + 1]] for p in pairs])
    start = np.concatenate([[0], np.cumsum([s[p + 1] - s[p] for p in pairs])]).astype(np.uint64)
    wh = np.tile(np.array(rref.IMAGE_WH * 2, np.uint32), (len(pairs), 1))
    K = np.tile(rref.K_MATRIX.reshape(1, 1, 3, 3), (len(pairs), 2, 1, 1))
    return xI, xJ, start, wh, K


def reference_robust(setting, p):
    g = gold()
    n = g["robust_n_inliers"][setting]
    lo = int(g["robust_n_inliers"][:setting].sum() + n[:p].sum())
    return dict(ok=bool(g["robust_ok"][setting, p]), precision=float(g["robust_precision"][setting, p]), E=g["robust_E"][setting, p].reshape(3, 3),
                pose=g["robust_pose"][setting, p], inliers=g["robust_inliers"][lo:lo + int(n[p])])


def check_robust_pinhole(setting, pairs=None):
    g = gold()
    tolerance, iterations = float(g["robust_settings"][setting][0]), int(g["robust_settings"][setting][1])
    n_all = len(g["robust_start"]) - 1
    pairs = list(range(n_all)) if pairs is None else list(pairs)
    xI, xJ, start, wh, K = robust_inputs(pairs)
    infos, mask, _ = rp.robust(xI, xJ, start, wh, K, tolerance, iterations)
    # the a-contrario part IS the filter's: same kernel, same bound (2.5 and 4.0 survive the square exactly)
    fmask, fres, _ = geofilter.filter_pairs_e(xI, xJ, start, wh, K, geofilter.GeometricFilter_EMatrix_AC(math.sqrt(tolerance), iterations))
    assert math.sqrt(tolerance) ** 2 == tolerance
    assert np.array_equal(mask, fmask)
    bI = np.zeros((len(xI), 3)); bJ = np.zeros((len(xI), 3))
    for q in range(len(pairs)):
        lo, hi = int(start[q]), int(start[q + 1])
        bI[lo:hi] = geofilter.pinhole_bearings(K[q, 0], xI[lo:hi]); bJ[lo:hi] = geofilter.pinhole_bearings(K[q, 1], xJ[lo:hi])
        i = infos[q]
        assert i.essential_matrix.tobytes() == fres["F"][q].tobytes() and i.found_residual_precision == fres["precision_robust"][q], pairs[q]
        assert i.n_acransac_inliers == int(fres["n_inliers"][q]) == len(i.vec_inliers) * bool(fres["ok"][q]) or not fres["ok"][q], pairs[q]
    # the pose part IS from_essential on that mask and E
    staged = rp.from_essential(fres["F"], bI, bJ, start, use=[np.flatnonzero(fmask[int(start[q]):int(start[q + 1])]) for q in range(len(pairs))])
    tol_pose, _ = tolerances()
    differing = 0
    for q, p in enumerate(pairs):
        i, s = infos[q], staged[q]
        if not fres["ok"][q]:
            assert not i.ok and not i.R.any() and len(i.selected) == 0, p
        else:
            assert i.ok == s.ok and i.cheirality == s.cheirality and np.array_equal(i.selected, s.selected), p
            assert i.R.tobytes() == s.R.tobytes() and i.t.tobytes() == s.t.tobytes() and i.center.tobytes() == s.center.tobytes() and i.points.tobytes() == s.points.tobytes(), p
        # against the compiled robustRelativePose
        ref = reference_robust(setting, p)
        if not np.array_equal(i.vec_inliers if fres["ok"][q] else np.zeros(0, np.uint32), ref["inliers"] if len(ref["inliers"]) >= 13 else np.zeros(0, np.uint32)):
            differing += 1
            continue
        assert i.ok == ref["ok"], (p, i.ok, ref["ok"])
        if i.ok:
            dE = float(np.abs(_geofilter_cases.normalised(i.essential_matrix) - _geofilter_cases.normalised(ref["E"])).max())
            assert dE < 1e-6, (p, dE)
            d_pose = float(np.abs(np.concatenate([i.R.ravel(), i.t, i.center]) - ref["pose"]).max())
            assert d_pose <= tol_pose + 10.0 * dE, (p, d_pose, tol_pose, dE)
            assert math.isclose(i.found_residual_precision, ref["precision"], rel_tol=1e-12), (p, i.found_residual_precision, ref["precision"])
    assert differing <= _geofilter_cases.allowed_differing(len(pairs), "e"), differing
    if n_all - 1 in pairs:   # the pair of 12 good correspondences
        last = infos[pairs.index(n_all - 1)]
        assert not last.ok and last.n_acransac_inliers < 13


# ---- 6. the robust entry, angular ----
def angular_pairs():
    """12 pairs of unit bearing vectors around the first camera (a spherical rig: z < 0 as well), 1e-3 rad of noise, 0 / 30 % outliers"""
    rng = np.random.default_rng([rref.SEED, 11])
    bI, bJ, start = [], [], [0]
    for n in (40, 60, 90, 120, 160, 200):
        for outliers in (0.0, 0.3):
            R, t = rref.general_motion(rng)
            d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
            a, b = rref.bearings(R, t, d * rng.uniform(3.0, 8.0, (n, 1)))
            a = a + 1e-3 * rng.standard_normal((n, 3)); b = b + 1e-3 * rng.standard_normal((n, 3))
            bad = rng.permutation(n)[:int(round(outliers * n))]
            b[bad] = rng.standard_normal((len(bad), 3))
            bI.append(a / np.linalg.norm(a, axis=1, keepdims=True)); bJ.append(b / np.linalg.norm(b, axis=1, keepdims=True)); start.append(start[-1] + n)
    assert (np.concatenate(bI)[:, 2] < 0).any()
    return np.concatenate(bI), np.concatenate(bJ), np.array(start, np.uint64)


def check_robust_angular(pairs=None, tolerance_deg=4.0, iterations=256):
    bI, bJ, start = angular_pairs()
    if pairs is not None:
        sel = np.concatenate([np.arange(int(start[p]), int(start[p + 1])) for p in pairs])
        start = np.concatenate([[0], np.cumsum([int(start[p + 1] - start[p]) for p in pairs])]).astype(np.uint64)
        bI, bJ = bI[sel], bJ[sel]
    n_pairs = len(start) - 1
    infos, mask, _ = rp.robust_angular(bI, bJ, start, tolerance_deg, iterations)
    fmask, fres, _ = geofilter.filter_pairs_angular(bI, bJ, start, geofilter.GeometricFilter_ESphericalMatrix_AC_Angular(tolerance_deg, iterations))
    used = []
    for q in range(n_pairs):
        lo, hi = int(start[q]), int(start[q + 1])
        i = infos[q]
        assert i.essential_matrix.tobytes() == fres["F"][q].tobytes() and i.n_acransac_inliers == int(fres["n_inliers"][q]), q
        assert i.found_residual_precision == fres["precision_robust"][q] * 180.0 / math.pi, q
        if i.n_acransac_inliers != 20:   # (at exactly 20 the two acceptance rules part, and so do the masks: check_twenty_inliers)
            assert np.array_equal(mask[lo:hi], fmask[lo:hi]), q
        used.append(np.flatnonzero(mask[lo:hi]))
    staged = rp.from_essential(fres["F"], bI, bJ, start, use=used)
    n_ok = 0
    for q in range(n_pairs):
        i, s = infos[q], staged[q]
        assert i.ok == s.ok and i.cheirality == s.cheirality and np.array_equal(i.selected, s.selected), q
        assert i.R.tobytes() == s.R.tobytes() and i.t.tobytes() == s.t.tobytes() and i.points.tobytes() == s.points.tobytes(), q
        n_ok += i.ok
    assert n_ok >= n_pairs // 2, n_ok
    return bI, bJ, start


def check_angular_pose_stage_against_oracle():
    """GPU, where oracle/_ref is present: the selected set against the compiled functor's second stage (E_ACRobust_Angular.hpp:126-143),
    given the mask and E of its own first stage - the pose stage and its plumbing against the reference, not the loop."""
    from tests import _oracle
    bI, bJ, start = angular_pairs()
    first = _oracle.ref_geofilter_angular(bI, bJ, start, 4.0, 256, pose_stage=False)
    second = _oracle.ref_geofilter_angular(bI, bJ, start, 4.0, 256, pose_stage=True)
    n_pairs = len(start) - 1
    used = [np.flatnonzero(first["mask"][int(start[p]):int(start[p + 1])]) for p in range(n_pairs)]
    infos = rp.from_essential(first["F"], bI, bJ, start, use=used)
    qualified = 0
    for p in range(n_pairs):
        if not (first["ok"][p] and second["ok"][p]):
            continue
        qualified += 1
        assert infos[p].ok, p
        assert np.array_equal(infos[p].selected, np.flatnonzero(second["mask"][int(start[p]):int(start[p + 1])])), p
    assert qualified >= 6, qualified


def check_twenty_inliers():
    """The acceptance rule at exactly 20 a-contrario inliers of the eight-point form, on the decision itself: 20 exact correspondences and
    10 bearings that belong to nothing. The filter's rule (n > 20) refuses the pair and clears its mask; robustRelativePose's
    (!(n < 20)) goes on to the cheirality stage - which must see mask and model of that pair."""
    rng = np.random.default_rng([rref.SEED, 21])   # (a draw on which the loop returns exactly the 20: the compiled sets are the filter's own)
    R, t = rref.general_motion(rng)
    a, b = rref.bearings(R, t, rref.points_in_front(R, t, 30, rng))
    b[20:] = rng.standard_normal((10, 3)); b[20:] /= np.linalg.norm(b[20:], axis=1, keepdims=True)
    infos, mask, _ = rp.robust_angular(a, b, [0, 30], 0.05, 256)
    fmask, fres, _ = geofilter.filter_pairs_angular(a, b, [0, 30], geofilter.GeometricFilter_ESphericalMatrix_AC_Angular(0.05, 256))
    assert int(fres["n_inliers"][0]) == 20 and not fres["ok"][0] and not fmask.any(), (fres["n_inliers"], fres["ok"])
    i = infos[0]
    assert i.n_acransac_inliers == 20 and np.array_equal(np.flatnonzero(mask), np.arange(20)) and i.ok
    assert i.essential_matrix.tobytes() == fres["F"][0].tobytes()
    assert np.array_equal(i.selected, np.arange(20)) and max(i.cheirality) == 20
    assert np.abs(i.R - R).max() < 1e-9 and np.abs(i.t - t).max() < 1e-9
    # the filter entry's own outputs are what they were: a second filter call after the robust one says the same
    fmask2, fres2, _ = geofilter.filter_pairs_angular(a, b, [0, 30], geofilter.GeometricFilter_ESphericalMatrix_AC_Angular(0.05, 256))
    assert not fmask2.any() and fres2.tobytes() == fres.tobytes()


# ---- the tiny scene of Relative_Pose_Engine ----
def check_tiny_scene():
    cs = stage_cases()
    c = cs[("ratio", 3, 10, 6)]
    start = [0, len(c["bI"])]
    info = rp.from_essential(c["E"][None], c["bI"], c["bJ"], start)
    assert info[0].ok
    scene = rp.tiny_scene_points(info, c["bI"], c["bJ"], start)
    tol_pose, tol_points = tolerances()
    assert scene[0].ok and np.array_equal(scene[0].selected, info[0].selected)
    assert np.abs(scene[0].R - info[0].R).max() <= tol_pose and np.abs(scene[0].points - info[0].points).max() <= tol_points * max(1.0, np.abs(info[0].points).max())
