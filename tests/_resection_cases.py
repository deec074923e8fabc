"""The cases of the resection tests, shared by tests/test_resection_emu_cpu.py (HIP emulation) and tests/test_resection_gpu.py (MI355X).

Yardstick: tests/_resection_ref.py, pinned to the compiled reference by tests/golden/resection_golden.npz (the two P3P solvers on 400
seeded samples; tests/golden/make_resection_golden.py). Tolerances are 1 000 x the spread recorded there between restatement and
reference, per solver ("Resection": three orders for contraction, OCML against glibc, grouping of sums).

Whole-run parity needs one piece of the device's run (tests/_resection_ref.py, UNORDERED_BELOW_PX): the three points of a sample have
residuals of 1e-13 px under their own model, their order at the head of the inlier list is rounding noise, that list becomes the sampling
pool, and the first later draw of one of them lets two correct implementations continue with different samples (left to itself the
restatement parts from the device in 17 of the 36 runs of the parity grid, in all nine at 4 096 iterations). So every device run here is
traced (test hook mvgx_resection_debug_trace: per iteration that found a better model, the head of its sorted list) and the restatement
takes the mutual order of those noise-level entries - nothing else - from the trace. It then draws the device's samples, and ok, iteration
count, the whole inlier list in its order, threshold, minNFA and pose are asserted for every run, full length included; a run is left out
only for a decision margin below the guard, and at most 5 % of the parity grid may be (check_left_out_cap)."""
import functools
import os

import numpy as np

from openmvg_amd import _capi, resection
from tests import _resection_ref as ref

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resection_golden.npz")
SOLVER_INDEX = {"ding": 0, "nordberg": 1}
W = 8   # the build's waves per workgroup (kResWaves)


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD_PATH))


def solver_tol(solver):
    return 1000.0 * float(gold()["solver_spread"][SOLVER_INDEX[solver]])


# The loop: the fixture records the reference's ACRANSAC (header-only, over the reference's Ding solver, adaptor of our own text) on the
# parity grid and, over the 27 of 36 runs in which it and the restatement return the same inlier list, the spread of minNFA (relative),
# of the threshold (relative) and of P. The guard on the restatement's decision margin is 1 000 x the NFA spread; the tolerances of
# minNFA, threshold and pose are 1 000 x the spread of each.
def loop_spread():
    nfa, err, P = (float(v) for v in gold()["loop_spread"])
    return nfa, err, P


def guard():
    return 1000.0 * loop_spread()[0]


# ---- solvers alone ----
NEEDED_BRANCHES = {
    "ding": {"ding swap 0-2", "ding swap 0-1", "ding no swap (a01 > a02)", "ding no swap (a01 <= a02)", "cubic c > 0", "cubic c < 0",
             "ding switch_12", "ding no switch_12"},
    "nordberg": {"nordberg |u1| < |u2|", "nordberg |u1| >= |u2|"},
}


def check_solver(solver):
    g = gold()
    s = SOLVER_INDEX[solver]
    B, X = g["bearings"], g["X"]
    truth = np.concatenate([g["R"], g["t"][:, :, None]], 2)
    hit = set()
    for i in range(len(B)):
        ref.SOLVERS[solver](B[i], X[i], None, hit)
    assert NEEDED_BRANCHES[solver] <= hit, f"branches not exercised by the fixture: {NEEDED_BRANCHES[solver] - hit}"
    Rt, count = resection.p3p(solver, B, X)
    assert np.array_equal(count, g["ref_count"][s]), "number of models"
    tol = solver_tol(solver)
    worst = float(np.abs(Rt - g["own_Rt"][s]).max())
    err = np.array([min((np.abs(Rt[i, m] - truth[i]).max() for m in range(count[i])), default=np.inf) for i in range(len(B))])
    bound = np.maximum(10.0 * g["ref_error"][s], tol)
    print(f"{solver}: largest |d(R|t)| against the restatement {worst:.3g} (tolerance {tol:.3g}); largest error of the best model {err.max():.3g}")
    assert worst <= tol
    assert np.all(err <= bound), f"best model off the generating pose: {err[err > bound]} against {bound[err > bound]}"
    assert np.all(Rt[np.arange(4)[None, :] >= count[:, None]] == 0.0)   # nothing written beyond the count


# ---- the loop ----
def run_device(problems, offset=0, **opts):
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
    return resection.localize(start, x2d, X3d, model, intr, **opts)


_RUNS = {}


def restated(key, pr, max_iteration):
    """the restatement's run of a problem, computed once"""
    k = (key, max_iteration)
    if k not in _RUNS:
        _RUNS[k] = ref.localize(pr["model"], pr["intr"], pr["x2d"], pr["X3d"], max_iteration=max_iteration)
    return _RUNS[k]


def same(a, b):
    """bit-identical results"""
    if a.ok != b.ok or a.error_max != b.error_max or a.min_nfa != b.min_nfa or not np.array_equal(a.inliers, b.inliers):
        return False
    return not a.ok or (np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and np.array_equal(a.C, b.C) and np.array_equal(a.P, b.P))


def check_self_consistent(pr, got):
    """the inliers are exactly the correspondences within the returned threshold under the returned model, in ascending residual"""
    if not len(got.inliers):
        assert not got.ok
        return
    assert got.ok == (len(got.inliers) > 7)
    assert len(set(got.inliers.tolist())) == len(got.inliers) and got.inliers.max() < len(pr["x2d"])
    if not got.ok:
        return
    assert np.abs(got.R @ got.R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(got.R) - 1.0) < 1e-12
    assert np.abs(got.C + got.R.T @ got.t).max() < 1e-12
    assert np.abs(np.c_[got.R, got.t] - got.P).max() < 1e-9   # the RQ of [R | t] gives R | t back: the solver's rotation is orthonormal to rounding
    n1 = ref.n1_of(pr["model"], pr["intr"])
    e = ref.residuals(pr["model"], pr["intr"], got.P, pr["x2d"], pr["X3d"])
    thr = (got.error_max * n1) ** 2
    g = guard()
    clear = np.abs(e - thr) > g * thr
    inl = np.zeros(len(e), bool)
    inl[got.inliers] = True
    assert np.array_equal(inl[clear], (e <= thr)[clear])
    assert abs(e[got.inliers[-1]] - thr) <= g * thr   # the threshold is the largest inlier residual
    px = np.sqrt(e[got.inliers]) / n1
    steps = np.diff(px)
    assert np.all(steps[px[1:] > ref.UNORDERED_BELOW_PX] >= -g * px[-1])   # ascending, up to the noise at the sample's own points


TRACE_EVENTS = 256   # iterations with a better model that a traced run can record (the runs here have up to 20)


def check_run(key, pr, max_iteration=4096, solver="ding", **forms):
    """one problem on the device, traced: self-consistent, and equal to the restatement that takes the order of noise-level residuals from
    the trace - unless the restatement's decision margin is below the guard. Returns (device result, restatement's run, whether the
    comparison was made)."""
    got, stats = run_device([pr], max_iteration=max_iteration, solver=solver, trace_events=TRACE_EVENTS, **forms)
    got = got[0]
    assert got.better_count <= TRACE_EVENTS and all(a[0] < b[0] for a, b in zip(got.better, got.better[1:]))
    want = ref.localize(pr["model"], pr["intr"], pr["x2d"], pr["X3d"], solver=ref.SOLVERS_BY_NAME[solver], max_iteration=max_iteration,
                        heads={it: head for it, _, head in got.better})
    check_self_consistent(pr, got)
    assert want.undecided_at is None
    kept = want.margin >= guard()
    if kept:
        compare(got, stats.n_iterations, want)
        assert [it for it, _, _ in got.better] == sorted({it for it, what in want.trace if what == "better"})   # the same iterations found a better model
    return got, want, kept


def compare(got, n_iterations, want):
    tol_nfa, tol_err, tol_P = (1000.0 * v for v in loop_spread())
    assert got.ok == want.ok and n_iterations == want.n_iterations
    # the inlier list, order included (want.unordered: noise-level entries the restatement had no order for - empty for a traced run)
    fixed = ~np.isin(want.inliers, sorted(want.unordered))
    assert len(got.inliers) == len(want.inliers) and np.array_equal(got.inliers[fixed], want.inliers[fixed]), "inlier list (order included)"
    assert set(got.inliers[~fixed].tolist()) == set(want.inliers[~fixed].tolist())
    assert got.min_nfa == want.min_nfa or abs(got.min_nfa - want.min_nfa) <= tol_nfa * max(1.0, abs(want.min_nfa))
    assert got.error_max == want.error_max or abs(got.error_max - want.error_max) <= tol_err * abs(want.error_max)
    if want.ok:
        for a, b in ((got.R, want.R), (got.t, want.t), (got.C, want.C), (got.P, want.P)):
            assert np.abs(a - b).max() <= tol_P * max(1.0, np.abs(b).max())


PARITY_MODELS = (ref.PINHOLE, ref.RADIAL3, ref.SPHERICAL)
PARITY_OUTLIERS = (0.0, 0.3, 0.6)
PARITY_ITERATIONS = (9, 10, 40, 4096)


def parity_problem(model, outliers):
    n = 60 + 7 * int(outliers * 10) + model
    return ref.problem(n, model, outliers, noise=0.5, seed=100 * model + int(outliers * 10))


_PARITY = {}   # (model, outliers, max_iteration) -> compared (False: left out for its margin)


def check_parity(model, max_iteration):
    for o in PARITY_OUTLIERS:
        if (model, o, max_iteration) in _PARITY:
            continue
        _, want, kept = check_run(("parity", model, o), parity_problem(model, o), max_iteration)
        _PARITY[(model, o, max_iteration)] = kept
        print(f"model {model} outliers {o} max_iteration {max_iteration}: {want.n_iterations} iterations, margin {want.margin:.3g} "
              f"({want.margin_where}), {'compared' if kept else 'LEFT OUT'}")


def check_left_out_cap():
    """at most 5 % of the parity grid may be left out for a margin below the guard (runs what test_loop_parity has not run yet)"""
    for model in PARITY_MODELS:
        for it in PARITY_ITERATIONS:
            check_parity(model, it)
    left_out = [k for k, kept in _PARITY.items() if not kept]
    print(f"left out: {len(left_out)} of {len(_PARITY)} {left_out}")
    assert len(_PARITY) == 36 and len(left_out) <= 0.05 * len(_PARITY)


def check_form_independence(model, outliers, max_iteration=4096):
    pr = parity_problem(model, outliers)
    n = len(pr["x2d"])
    base, st0 = run_device([pr], max_iteration=max_iteration)
    for forms in (dict(waves_ahead=1), dict(waves_ahead=2), dict(waves_ahead=W), dict(global_above=n - 1), dict(global_above=n),
                  dict(global_above=n - 1, waves_ahead=3)):
        got, st = run_device([pr], max_iteration=max_iteration, **forms)
        assert same(got[0], base[0]) and st.n_iterations == st0.n_iterations and st.n_models == st0.n_models, f"form {forms} changes the result"
    check_self_consistent(pr, base[0])


# ---- form edges ----
def clean_problem(n, seed, noise=0.01):
    return ref.problem(n, ref.PINHOLE, 0.0, noise=noise, seed=seed)


def check_tiny():
    """n = 3: not ok, nothing written; n = 4: the only k is 4"""
    got, stats = run_device([clean_problem(3, 1)])
    assert not got[0].ok and len(got[0].inliers) == 0 and got[0].error_max == 0.0 and got[0].min_nfa == 0.0 and stats.n_iterations == 0
    pr = clean_problem(4, 2)
    got, want, _ = check_run("n4", pr, 64)
    assert not got.ok and len(got.inliers) in (0, 4) and len(want.inliers) in (0, 4)


def check_seven_and_eight():
    """all points fit: seven inliers are too few (7 > 7.5 is false), eight are enough"""
    got7, _, _ = check_run("n7", clean_problem(7, 3), 64)
    got8, _, _ = check_run("n8", clean_problem(8, 4), 64)
    assert len(got7.inliers) == 7 and not got7.ok and got7.error_max < 0.1
    assert len(got8.inliers) == 8 and got8.ok and got8.error_max < 0.1


def check_size_edge(n):
    """lane-stride and sort-padding edges: 63, 64, 65, 128, 129 correspondences, in LDS and in global scratch, bit for bit the same"""
    pr = ref.problem(n, ref.PINHOLE, 0.3, seed=1000 + n)
    got, _, _ = check_run(("size", n), pr, 40)
    assert got.ok and not pr["is_outlier"][got.inliers].any()
    other, _ = run_device([pr], max_iteration=40, global_above=n - 1)
    assert same(other[0], got)


def check_iteration_edge(max_iteration):
    """max_iteration = 1, 9 (no reserve), 10 (a reserve of one) and 4 096"""
    pr = ref.problem(50, ref.PINHOLE, 0.3, seed=77)
    got, want, kept = check_run("iter-edge", pr, max_iteration)
    assert kept
    if max_iteration == 1:
        assert not got.ok   # one sample of a 30 % outlier problem, and NFA >= 0 or not: the reserve is 0, nothing is adopted


def check_tied_residuals():
    """every correspondence twice: pairs of residuals equal to the bit, which order by index (std::pair<double, uint32_t>)"""
    half = ref.problem(24, ref.PINHOLE, 0.25, seed=34)   # (a seed whose first sample is three inliers)
    pr = dict(half, x2d=np.concatenate([half["x2d"], half["x2d"]]), X3d=np.concatenate([half["X3d"], half["X3d"]]),
              is_outlier=np.concatenate([half["is_outlier"]] * 2))
    got, want, decided = check_run("tied", pr, 1)   # one iteration: with every point twice, any later draw meets a point of the first sample
    assert decided and got.ok
    e = ref.residuals(pr["model"], pr["intr"], got.P, pr["x2d"], pr["X3d"])
    noise = set(np.flatnonzero(np.sqrt(e) / ref.n1_of(pr["model"], pr["intr"]) < ref.UNORDERED_BELOW_PX).tolist())   # the sample's own points and their copies
    pos = {int(v): i for i, v in enumerate(got.inliers)}
    pairs = [(i, i + 24) for i in range(24) if i in pos and i + 24 in pos]
    assert len(pairs) >= 12 and all(pos[b] > pos[a] for a, b in pairs)   # equal residuals: the lower index first ...
    # ... and at once, wherever the residual is not shared with another pair (two of the sample's own points can both be exactly 0)
    assert all(pos[b] == pos[a] + 1 for a, b in pairs if a not in noise)


def check_all_outliers():
    """nothing but uniform pixels: minNFA >= 0, the result is cleared"""
    pr = ref.problem(40, ref.PINHOLE, 1.0, seed=5)
    got, want, _ = check_run("all-outliers", pr, 40)
    assert want.min_nfa >= 0 and not want.ok and len(want.inliers) == 0
    assert got.min_nfa >= 0 and not got.ok and len(got.inliers) == 0


def check_no_model_at_all():
    """collinear points: no sample gives a finite model, vec_inliers stays empty and the end-of-nIter branch extends the loop
    (++nIter; --nIterReserve) until the reserve is used up"""
    pr = ref.problem(12, ref.PINHOLE, 0.0, seed=6)
    pr["X3d"] = np.stack([np.arange(12.0), 2.0 * np.arange(12.0), np.full(12, 3.0)], 1)
    want = restated("collinear", pr, 40)
    assert ("extend" in [w for _, w in want.trace]) and want.n_models == 0 and want.n_iterations == 40
    got, stats = run_device([pr], max_iteration=40)
    assert not got[0].ok and len(got[0].inliers) == 0 and stats.n_iterations == 40 and stats.n_models == 0
    assert got[0].min_nfa == np.inf and got[0].error_max == np.inf


def check_mixed_batch():
    """every edge in one call, an empty problem in the middle, start with an offset into larger arrays: each result is the single call's"""
    prs = [clean_problem(3, 1), ref.problem(65, ref.PINHOLE, 0.3, seed=1065), clean_problem(7, 3), None, ref.problem(40, ref.PINHOLE, 1.0, seed=5),
           parity_problem(ref.SPHERICAL, 0.3), clean_problem(8, 4), ref.problem(129, ref.PINHOLE, 0.3, seed=1129), parity_problem(ref.RADIAL3, 0.6)]
    batch, stats = run_device(prs, offset=5, max_iteration=40, global_above=100)
    assert stats.n_problems == len(prs)
    total = 0
    for p, b in zip(prs, batch):
        if p is None:
            assert not b.ok and len(b.inliers) == 0
            continue
        single, st = run_device([p], max_iteration=40, global_above=100)
        assert same(single[0], b)
        total += st.n_iterations
    assert stats.n_iterations == total


def check_arguments():
    pr = parity_problem(ref.PINHOLE, 0.3)

    def call(problems=(pr,), **kw):
        try:
            run_device(list(problems), **kw)
        except _capi.MvgxError as e:
            return e.code
        return _capi.MVGX_OK

    assert call(max_iteration=9) == _capi.MVGX_OK
    for solver in ("dlt6", "ke", "kneip", "up2p"):
        assert call(solver=solver) == _capi.MVGX_ERR_UNSUPPORTED
    assert call(error_max=4.0) == _capi.MVGX_ERR_UNSUPPORTED
    assert call(problems=(dict(pr, model=6),)) == _capi.MVGX_ERR_UNSUPPORTED
    n = len(pr["x2d"])
    try:
        resection.localize(np.array([0, n, n - 1], np.uint64), pr["x2d"], pr["X3d"], [1, 1], [pr["intr"]] * 2)
        code = _capi.MVGX_OK
    except _capi.MvgxError as e:
        code = e.code
    assert code == _capi.MVGX_ERR_ARG
    o = resection.default_options()
    assert (o.solver, o.max_iteration, o.error_max, o.waves_ahead, o.global_above) == (4, 4096, np.inf, 0, 0)


def check_nordberg_loop():
    """the loop over the other solver"""
    pr = parity_problem(ref.PINHOLE, 0.3)
    got, _, kept = check_run("nordberg", pr, 200, solver="nordberg")
    assert kept and got.ok


def check_pose_row():
    pr = parity_problem(ref.PINHOLE, 0.0)
    got, _ = run_device([pr], max_iteration=40)
    row = resection.pose_row(got[0])
    from tests import _triangulation_ref as tri
    assert np.abs(np.array(tri.rotation(row[:3])) - got[0].R).max() < 1e-12 and np.array_equal(row[3:], got[0].t)
    assert np.abs(got[0].R - pr["R"]).max() < 5e-3 and np.abs(got[0].t - pr["t"]).max() < 5e-2   # 0.5 px noise on 60 points
