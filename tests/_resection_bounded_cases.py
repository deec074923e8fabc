"""The cases of the bounded resection tests (mvgx_resection_localize_bounded), shared by tests/test_resection_bounded_emu_cpu.py (HIP
emulation) and tests/test_resection_bounded_gpu.py (MI355X).

Yardstick: tests/_resection_bounded_ref.py, pinned to the compiled reference by tests/golden/resection_bounded_golden.npz
(tests/golden/make_resection_bounded_golden.py: the reference's ACRANSAC with a finite precision on the 108 runs of PARITY_GRID). The
fixture records the spreads between restatement and compiled reference: |dP|, the relative residual, and whether minNFA and threshold
are equal to the bit. Tolerances are 1 000 x the spread; the guard on a run's decision margin is 1 000 x the relative residual spread.
A run whose margin is below the guard is left out of the comparison; at most 5 % of the grid may be (check_left_out_cap).

No trace is needed in this form: the inlier list is in index order, so the pool a list becomes does not depend on rounding noise."""
import functools
import math
import os

import numpy as np

from openmvg_amd import _capi, resection
from tests import _resection_bounded_ref as bref
from tests import _resection_ref as ref

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resection_bounded_golden.npz")
W = 8              # the build's waves per workgroup (kResWaves)
LDS_MAX_N = 8192   # the build's largest problem whose tables live in LDS (kResBLdsMaxN)

PARITY_MODELS = (ref.PINHOLE, ref.RADIAL3, ref.SPHERICAL)
PARITY_OUTLIERS = (0.0, 0.3, 0.6)
PARITY_ITERATIONS = (9, 10, 40, 4096)
PARITY_ERROR_MAX = (1.0, 4.0, 16.0)
PARITY_GRID = [(m, o, it, em) for it in PARITY_ITERATIONS for m in PARITY_MODELS for o in PARITY_OUTLIERS for em in PARITY_ERROR_MAX]


def parity_problem(model, outliers):
    """the problems of tests/_resection_cases.py's parity grid"""
    n = 60 + 7 * int(outliers * 10) + model
    return ref.problem(n, model, outliers, noise=0.5, seed=100 * model + int(outliers * 10))


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD_PATH))


def spreads():
    """(|dP|, relative residual, relative minNFA difference, relative threshold difference) restatement - compiled reference; the last two
    are 0 when the two are equal to the bit in every run"""
    return tuple(float(v) for v in gold()["spread"])


def guard():
    return 1000.0 * spreads()[1]


def gold_run(index):
    g = gold()
    at = int(np.sum(g["n_inliers"][:index]))
    ra = int(np.sum(g["n_residuals"][:index]))
    return dict(inliers=g["inliers"][at:at + int(g["n_inliers"][index])], error_max=float(g["error_max"][index]), min_nfa=float(g["min_nfa"][index]),
                P=g["P"][index], residuals=g["residuals"][ra:ra + int(g["n_residuals"][index])])


def close_or_equal(a, b, spread):
    """equal to the bit where the fixture found restatement and reference equal to the bit; else within 1 000 x the recorded difference"""
    return a == b or (spread > 0.0 and abs(a - b) <= 1000.0 * spread * max(1.0, abs(b)))


# ---- the device ----
def run_device(problems, error_max, offset=0, **opts):
    """problems: list of dicts of ref.problem (or None: an empty problem). offset: rows of padding before the first problem."""
    ns = [0 if p is None else len(p["x2d"]) for p in problems]
    start = np.concatenate([[offset], offset + np.cumsum(ns)]).astype(np.uint64)
    x2d = np.full((offset + sum(ns) + 3, 2), np.nan)
    X3d = np.full((offset + sum(ns) + 3, 3), np.nan)
    for p, lo in zip(problems, start[:-1]):
        if p is not None:
            x2d[int(lo):int(lo) + len(p["x2d"])] = p["x2d"]
            X3d[int(lo):int(lo) + len(p["x2d"])] = p["X3d"]
    model = [ref.PINHOLE if p is None else p["model"] for p in problems]
    intr = [np.array([1000.0, 0, 0, 0, 0, 0, 0, 0]) if p is None else p["intr"] for p in problems]
    return resection.localize_bounded(start, x2d, X3d, model, intr, error_max, **opts)


_RUNS = {}


def restated(key, pr, error_max, max_iteration, solver="ding"):
    """the restatement's run of a problem, computed once and left unchanged"""
    k = (key, error_max, max_iteration, solver)
    if k not in _RUNS:
        _RUNS[k] = bref.localize_bounded(pr["model"], pr["intr"], pr["x2d"], pr["X3d"], error_max, solver=ref.SOLVERS_BY_NAME[solver],
                                         max_iteration=max_iteration)
    return _RUNS[k]


def same(a, b):
    """bit-identical results"""
    if a.ok != b.ok or a.error_max != b.error_max or a.min_nfa != b.min_nfa or not np.array_equal(a.inliers, b.inliers):
        return False
    return not a.ok or (np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and np.array_equal(a.C, b.C) and np.array_equal(a.P, b.P))


def check_self_consistent(pr, got, error_max):
    """the threshold is one of the bin values 1..19 of the bound; the inliers are exactly {i : e_i <= thr} under the returned model, ascending"""
    if not len(got.inliers):
        assert not got.ok
        return
    assert got.ok == (len(got.inliers) > 7)
    assert np.all(np.diff(got.inliers.astype(np.int64)) > 0) and got.inliers.max() < len(pr["x2d"])
    n1 = ref.n1_of(pr["model"], pr["intr"])
    max_threshold = bref.bound_constants(pr["model"], pr["intr"], error_max)[0]
    thr = (got.error_max * n1) ** 2
    step = thr / max_threshold * 19.0
    assert abs(step - round(step)) < 1e-9 and 1 <= round(step) <= 19, f"threshold {got.error_max} px is no bin value of the bound {error_max} px"
    if not got.ok:
        return
    assert np.abs(got.R @ got.R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(got.R) - 1.0) < 1e-12
    assert np.abs(got.C + got.R.T @ got.t).max() < 1e-12
    e = ref.residuals(pr["model"], pr["intr"], got.P, pr["x2d"], pr["X3d"])
    clear = np.abs(e - thr) > guard() * thr   # (this residual is the restatement's arithmetic, not the device's)
    inl = np.zeros(len(e), bool)
    inl[got.inliers] = True
    assert np.array_equal(inl[clear], (e <= thr)[clear])


def compare(got, stats, want):
    tol_P = 1000.0 * spreads()[0]
    assert got.ok == want.ok and stats.n_iterations == want.n_iterations and stats.n_models == want.n_models
    assert np.array_equal(got.inliers, want.inliers), "inlier list"
    assert close_or_equal(got.min_nfa, want.min_nfa, spreads()[2]), (got.min_nfa, want.min_nfa)
    assert close_or_equal(got.error_max, want.error_max, spreads()[3]), (got.error_max, want.error_max)
    if want.ok:
        for a, b in ((got.R, want.R), (got.t, want.t), (got.C, want.C), (got.P, want.P)):
            assert np.abs(a - b).max() <= tol_P * max(1.0, np.abs(b).max())


def check_run(key, pr, error_max, max_iteration=4096, solver="ding", **forms):
    """one problem on the device: self-consistent, and equal to the restatement unless its decision margin is below the guard. Returns
    (device result, stats, restatement's run, whether the comparison was made)."""
    got, stats = run_device([pr], error_max, max_iteration=max_iteration, solver=solver, **forms)
    got = got[0]
    want = restated(key, pr, error_max, max_iteration, solver)
    check_self_consistent(pr, got, error_max)
    kept = want.margin >= guard()
    if kept:
        compare(got, stats, want)
    return got, stats, want, kept


# ---- parity ----
_PARITY = {}   # (model, outliers, max_iteration, error_max) -> compared (False: left out for its margin)


def check_parity(model, max_iteration):
    for o in PARITY_OUTLIERS:
        for em in PARITY_ERROR_MAX:
            if (model, o, max_iteration, em) in _PARITY:
                continue
            _, _, want, kept = check_run(("parity", model, o), parity_problem(model, o), em, max_iteration)
            _PARITY[(model, o, max_iteration, em)] = kept
            print(f"model {model} outliers {o} max_iteration {max_iteration} error_max {em}: {want.n_iterations} iterations, switch at {want.switch_at}, "
                  f"margin {want.margin:.3g} ({want.margin_where}), {'compared' if kept else 'LEFT OUT'}")


def check_left_out_cap():
    """at most 5 % of the 108 runs may be left out for a margin below the guard (runs what test_loop_parity has not run yet)"""
    for model in PARITY_MODELS:
        for it in PARITY_ITERATIONS:
            check_parity(model, it)
    left_out = [k for k, kept in _PARITY.items() if not kept]
    print(f"left out: {len(left_out)} of {len(_PARITY)} {left_out}")
    assert len(_PARITY) == len(PARITY_GRID) == 108 and len(left_out) <= 0.05 * len(_PARITY)


def check_form_independence(model, outliers, max_iteration, error_max=4.0):
    """waves_ahead 1, 2, 8 and both storage forms return identical bits"""
    pr = parity_problem(model, outliers)
    n = len(pr["x2d"])
    base, st0 = run_device([pr], error_max, max_iteration=max_iteration)
    for forms in (dict(waves_ahead=1), dict(waves_ahead=2), dict(waves_ahead=W), dict(global_above=n - 1), dict(global_above=n),
                  dict(global_above=n - 1, waves_ahead=3)):
        got, st = run_device([pr], error_max, max_iteration=max_iteration, **forms)
        assert same(got[0], base[0]) and st.n_iterations == st0.n_iterations and st.n_models == st0.n_models, f"form {forms} changes the result"
    check_self_consistent(pr, base[0], error_max)
    return base[0]


def check_switch_mid_block():
    """60 % outliers: the a-contrario mode turns on at iteration 12 - 32, inside a block of eight, never on a block's first iteration for
    every one of the three problems"""
    at = []
    for model in PARITY_MODELS:
        want = restated(("parity", model, 0.6), parity_problem(model, 0.6), 4.0, 400)
        assert want.switch_at is not None and 12 <= want.switch_at <= 32
        at.append(want.switch_at)
        got = check_form_independence(model, 0.6, 400)
        assert got.ok
    assert any(a % W for a in at), at


# ---- the switch and the early exit ----
def few_inliers_problem(n_inliers, seed):
    """n_inliers correspondences of one pose (0.01 px noise) among 12 uniform ones"""
    n = n_inliers + 12
    pr = ref.problem(n, ref.PINHOLE, 12.0 / n, noise=0.01, seed=seed)
    assert int(pr["is_outlier"].sum()) == 12
    return pr


def check_switch_threshold():
    """exactly 7 correspondences inside the bound: 7 > 7.5 is false, the mode never turns on, the loop exits early; exactly 8: it turns on"""
    pr7, pr8 = few_inliers_problem(7, 7), few_inliers_problem(8, 8)
    got7, st7, want7, kept7 = check_run("seven", pr7, 1.0, 400)
    assert kept7 and want7.switch_at is None and st7.n_iterations == 2 * 40 + 2
    assert not got7.ok and len(got7.inliers) == 0 and got7.min_nfa == math.inf and got7.error_max == math.inf
    got8, st8, want8, kept8 = check_run("eight", pr8, 1.0, 400)
    assert kept8 and want8.switch_at is not None
    assert got8.ok and np.array_equal(got8.inliers, np.flatnonzero(~pr8["is_outlier"]))


EARLY_EXIT = {1: 1, 9: 2, 10: 4, 40: 10, 4096: 820}   # 2 (max_iteration / 10) + 2, or max_iteration where the loop is shorter


def check_early_exit(max_iteration):
    """nothing but uniform pixels: no model ever has 8 residuals inside the bound"""
    pr = ref.problem(40, ref.PINHOLE, 1.0, seed=5)
    got, stats, want, kept = check_run("all-outliers", pr, 4.0, max_iteration)
    assert kept and want.switch_at is None
    assert stats.n_iterations == EARLY_EXIT[max_iteration]
    assert not got.ok and len(got.inliers) == 0 and got.min_nfa == math.inf and got.error_max == math.inf


def check_epsilon_gate():
    """a bound so small that every bin value is <= FLT_EPSILON (0.3 px at f ~ 1 000: maxThreshold ~ 9e-8): the mode turns on, no NFA is ever
    produced, vec_inliers stays empty and the end-of-nIter branch extends the loop until the reserve is used up. At 1 px only the bins
    from 3 up pass the gate."""
    pr = ref.problem(30, ref.PINHOLE, 0.0, noise=0.01, seed=11)
    consts = bref.bound_constants(pr["model"], pr["intr"], 0.3)
    assert max(consts[2]) <= ref.FLT_EPS
    got, stats, want, kept = check_run("eps", pr, 0.3, 40)
    assert kept and want.switch_at is not None and want.n_nfa == 0 and "extend" in [w for _, w in want.trace]
    assert stats.n_iterations == 40 and not got.ok and len(got.inliers) == 0 and got.min_nfa == math.inf
    values = bref.bound_constants(pr["model"], pr["intr"], 1.0)[2]
    assert [b for b in range(bref.N_BINS) if values[b] > ref.FLT_EPS] == list(range(3, 20))
    got, stats, want, kept = check_run("eps", pr, 1.0, 40)
    assert kept and want.n_nfa > 0
    if len(got.inliers):
        n1 = ref.n1_of(pr["model"], pr["intr"])
        assert round((got.error_max * n1) ** 2 / values[19] * 19.0) >= 3


# ---- form edges ----
def check_size_edge(n):
    """the strides of the residual passes (64) and of the ordered compaction (512), and the storage switch: bit for bit the same in LDS
    and in global scratch where both forms take the size"""
    pr = ref.problem(n, ref.PINHOLE, 0.3, seed=1000 + n)
    got, stats, want, kept = check_run(("size", n), pr, 4.0, 40)
    if n >= 63:
        assert kept and got.ok and not pr["is_outlier"][got.inliers].any()
    else:
        assert not got.ok and stats.n_iterations == EARLY_EXIT[40]   # four correspondences never give eight inside the bound
    if n <= LDS_MAX_N:
        other, st = run_device([pr], 4.0, max_iteration=40, global_above=n - 1)
        assert same(other[0], got) and st.n_iterations == stats.n_iterations and st.n_models == stats.n_models


def check_nordberg_loop():
    """the loop over the other solver"""
    pr = parity_problem(ref.PINHOLE, 0.3)
    got, _, _, kept = check_run("nordberg", pr, 4.0, 200, solver="nordberg")
    assert kept and got.ok


def check_mixed_batch():
    """several edges in one call, an empty problem in the middle, start with an offset into larger arrays: each result is the single call's"""
    prs = [ref.problem(3, ref.PINHOLE, 0.0, seed=1), ref.problem(65, ref.PINHOLE, 0.3, seed=1065), few_inliers_problem(7, 7), None,
           ref.problem(40, ref.PINHOLE, 1.0, seed=5), parity_problem(ref.SPHERICAL, 0.3), few_inliers_problem(8, 8),
           ref.problem(129, ref.PINHOLE, 0.3, seed=1129), parity_problem(ref.RADIAL3, 0.6)]
    batch, stats = run_device(prs, 4.0, offset=5, max_iteration=400, global_above=100)
    assert stats.n_problems == len(prs)
    total = 0
    for p, b in zip(prs, batch):
        if p is None or len(p["x2d"]) <= 3:
            assert not b.ok and len(b.inliers) == 0 and b.error_max == 0.0 and b.min_nfa == 0.0
            continue
        single, st = run_device([p], 4.0, max_iteration=400, global_above=100)
        assert same(single[0], b)
        check_self_consistent(p, b, 4.0)
        total += st.n_iterations
    assert stats.n_iterations == total


def check_arguments():
    pr = parity_problem(ref.PINHOLE, 0.3)

    def call(error_max=4.0, **kw):
        try:
            run_device([pr], error_max, **kw)
        except _capi.MvgxError as e:
            return e.code
        return _capi.MVGX_OK

    assert call(max_iteration=9) == _capi.MVGX_OK
    for em in (math.inf, 0.0, -1.0, math.nan):
        assert call(error_max=em) == _capi.MVGX_ERR_ARG
    for solver in ("dlt6", "ke", "kneip", "up2p"):
        assert call(solver=solver) == _capi.MVGX_ERR_UNSUPPORTED
    n = len(pr["x2d"])
    try:   # the old entry still refuses a finite bound, and names the new one
        resection.localize([0, n], pr["x2d"], pr["X3d"], [pr["model"]], [pr["intr"]], error_max=4.0)
        code, text = _capi.MVGX_OK, ""
    except _capi.MvgxError as e:
        code, text = e.code, str(e)
    assert code == _capi.MVGX_ERR_UNSUPPORTED and "mvgx_resection_localize_bounded" in text
