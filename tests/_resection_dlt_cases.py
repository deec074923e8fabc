"""The cases of the uncalibrated resection tests (mvgx_resection_localize_uncalibrated), shared by tests/test_resection_dlt_emu_cpu.py (HIP
emulation) and tests/test_resection_dlt_gpu.py (MI355X).

Yardstick: tests/_resection_dlt_ref.py, pinned to the compiled reference by tests/golden/resection_dlt_golden.npz
(tests/golden/make_resection_dlt_golden.py: SixPointResectionSolver::Solve on 461 seeded samples, ACRANSAC through the reference's own
ACKernelAdaptorResection on the 36 runs of the parity grid). Every tolerance is 1 000 x the spread recorded there between restatement and
reference; the guard on a decision margin is 1 000 x the NFA spread. None is typed in here.

Every device run of the loop is traced (mvgx_resection_debug_trace) and the restatement takes the mutual order of noise-level residuals
from the trace, as tests/_resection_cases.py does; with 0.5 px of noise a six-point sample's own residuals are 2e-3 px and more, so the
mechanism only acts on the near-noiseless problems of the small-n cases."""
import functools
import os

import numpy as np

from openmvg_amd import _capi, resection
from tests import _resection_dlt_ref as dref
from tests import _resection_ref as ref

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resection_dlt_golden.npz")
W = 8             # the build's waves per workgroup (kResWaves)
LDS_MAX_N = 1024  # the largest n of the LDS form (kDltLdsMaxN; DESIGN.md derives it)
SWEEP_CAP = 30    # kDltSweepCap
WH = dref.IMAGE_WH
TRACE_EVENTS = 256


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD_PATH))


def solver_tol():
    """(relative |dP|, relative ratio)"""
    return tuple(1000.0 * float(v) for v in gold()["solver_spread"])


def loop_tol():
    """(relative NFA, relative threshold, relative |dP|)"""
    return tuple(1000.0 * float(v) for v in gold()["loop_spread"])


def guard():
    return 1000.0 * float(gold()["loop_spread"][0])


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(b).max()))


# ---- the solver alone ----
# "K(2,2) < 0" is not among them: the first Givens step leaves K(2,2) = -hypot(.), the second +hypot(.), so that fix is taken only when
# P(2,0) is exactly zero, which a null vector out of a singular value iteration never is.
NEEDED_BRANCHES = {"ratio rejected", "depth rejected", "in front", "det R < 0", "K(1,1) < 0", "K(0,0) < 0"}


def check_solver():
    g = gold()
    x, X = g["x_norm"], g["X"]
    hit, margin = set(), np.zeros(len(x))
    for i in range(len(x)):
        mg = ref.Margin()
        dref.six_point(x[i], X[i], mg, hit)
        margin[i] = mg.value
    assert NEEDED_BRANCHES <= hit, f"branches not exercised by the fixture: {NEEDED_BRANCHES - hit}"
    assert all(np.any(g["group"] == k) for k in range(5)) and set(g["ref_count"][g["group"] == 2].tolist()) == {0}   # one point behind: never a model
    P, count, ratio, sweeps = resection.dlt6(x, X)
    decided = margin >= guard()
    assert decided.sum() >= 0.95 * len(x)
    assert np.array_equal(count[decided], g["ref_count"][decided]), "number of models"
    tol_P, tol_ratio = solver_tol()
    both = (count == 1) & (g["ref_count"] == 1)
    worst = max(rel(P[i], g["own_P"][i]) for i in np.flatnonzero(both))
    worst_ratio = float(np.abs(ratio / g["own_ratio"] - 1.0).max())
    print(f"dlt6: {int(count.sum())} models of {len(x)}; largest relative |dP| against the restatement {worst:.3g} (tolerance {tol_P:.3g}), of the ratio "
          f"{worst_ratio:.3g} (tolerance {tol_ratio:.3g}); sweeps {sweeps.min()} .. {sweeps.max()}")
    assert worst <= tol_P and worst_ratio <= tol_ratio
    assert sweeps.max() < SWEEP_CAP and sweeps.min() >= 2
    assert np.all(P[count == 0] == 0.0)   # nothing without a model
    assert np.all(P[count == 1][:, 2, 3] == 1.0)   # P /= P(2,3)


# ---- the loop ----
def run_device(problems, offset=0, wh=None, **opts):
    """problems: list of dicts of ref.problem (or None: an empty problem). offset: rows of padding before the first problem."""
    ns = [0 if p is None else len(p["x2d"]) for p in problems]
    start = np.concatenate([[offset], offset + np.cumsum(ns)]).astype(np.uint64)
    x2d = np.full((offset + sum(ns) + 3, 2), np.nan)
    X3d = np.full((offset + sum(ns) + 3, 3), np.nan)
    for p, lo in zip(problems, start[:-1]):
        if p is not None:
            x2d[int(lo):int(lo) + len(p["x2d"])] = p["x2d"]
            X3d[int(lo):int(lo) + len(p["x2d"])] = p["X3d"]
    return resection.localize_uncalibrated(start, x2d, X3d, [WH] * len(problems) if wh is None else wh, **opts)


def same(a, b):
    """bit-identical results"""
    if a.ok != b.ok or a.error_max != b.error_max or a.min_nfa != b.min_nfa or not np.array_equal(a.inliers, b.inliers):
        return False
    return not a.ok or all(np.array_equal(u, v) for u, v in ((a.R, b.R), (a.t, b.t), (a.C, b.C), (a.P, b.P), (a.K, b.K)))


def check_self_consistent(pr, got, wh=WH):
    """the inliers are exactly the correspondences within the returned threshold under the returned P, in ascending residual; K is a
    calibration matrix; K [R | t] reproduces P up to scale"""
    if not len(got.inliers):
        assert not got.ok
        return
    assert got.ok == (len(got.inliers) > 15)
    assert len(set(got.inliers.tolist())) == len(got.inliers) and got.inliers.max() < len(pr["x2d"])
    if not got.ok:
        return
    K = got.K
    assert max(abs(K[2, 0]), abs(K[2, 1]), abs(K[1, 0])) <= 1e-12 * K[0, 0] and K[0, 0] > 0 and K[1, 1] > 0 and K[2, 2] == 1.0
    assert np.abs(got.R @ got.R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(got.R) - 1.0) < 1e-12
    assert np.abs(got.C + got.R.T @ got.t).max() < 1e-12
    KRt = K @ np.c_[got.R, got.t]
    scale = got.P[2, 3] / KRt[2, 3]
    assert np.abs(KRt * scale - got.P).max() <= 1e-9 * np.abs(got.P).max()
    # the pixel residuals under the returned (unnormalised) P: the normalisation is a similarity, so they are the normalised ones / dNorm
    p = pr["X3d"] @ got.P[:, :3].T + got.P[:, 3]
    with np.errstate(all="ignore"):
        e = ((pr["x2d"] - p[:, :2] / p[:, 2:]) ** 2).sum(1)
    e[~np.isfinite(e)] = np.inf
    thr = got.error_max ** 2
    g = max(guard(), 1e-9)   # (P went through the unnormalisation: its own rounding, relative 1e-13 of entries up to 1e3)
    clear = np.abs(e - thr) > g * thr
    inl = np.zeros(len(e), bool)
    inl[got.inliers] = True
    assert np.array_equal(inl[clear], (e <= thr)[clear])
    assert abs(e[got.inliers[-1]] - thr) <= g * thr   # the threshold is the largest inlier residual
    px = np.sqrt(e[got.inliers])
    steps = np.diff(px)
    assert np.all(steps[px[1:] > ref.UNORDERED_BELOW_PX] >= -g * px[-1])


def compare(got, n_iterations, n_models, want):
    tol_nfa, tol_err, tol_P = loop_tol()
    assert got.ok == want.ok and n_iterations == want.n_iterations and n_models == want.n_models
    fixed = ~np.isin(want.inliers, sorted(want.unordered))
    assert len(got.inliers) == len(want.inliers) and np.array_equal(got.inliers[fixed], want.inliers[fixed]), "inlier list (order included)"
    assert set(got.inliers[~fixed].tolist()) == set(want.inliers[~fixed].tolist())
    assert got.min_nfa == want.min_nfa or abs(got.min_nfa - want.min_nfa) <= tol_nfa * max(1.0, abs(want.min_nfa))
    assert got.error_max == want.error_max or abs(got.error_max - want.error_max) <= tol_err * abs(want.error_max)
    if want.ok:
        for a, b in ((got.R, want.R), (got.t, want.t), (got.C, want.C), (got.P, want.P), (got.K, want.K)):
            assert rel(a, b) <= tol_P


def check_run(pr, max_iteration=4096, wh=WH, **forms):
    """one problem on the device, traced: self-consistent, and equal to the restatement - unless the restatement's decision margin is
    below the guard. Returns (device result, restatement's run, whether the comparison was made)."""
    got, stats = run_device([pr], wh=[wh], max_iteration=max_iteration, trace_events=TRACE_EVENTS, **forms)
    got = got[0]
    assert got.better_count <= TRACE_EVENTS and all(a[0] < b[0] for a, b in zip(got.better, got.better[1:]))
    want = dref.localize(pr["x2d"], pr["X3d"], wh, max_iteration=max_iteration, heads={it: head for it, _, head in got.better})
    check_self_consistent(pr, got, wh)
    assert want.undecided_at is None
    kept = want.margin >= guard()
    if kept:
        compare(got, stats.n_iterations, stats.n_models, want)
        assert [it for it, _, _ in got.better] == sorted({it for it, what in want.trace if what == "better"})
    return got, want, kept


PARITY_OUTLIERS = (0.0, 0.3, 0.6)
PARITY_S = (1, 2, 3)
PARITY_ITERATIONS = (9, 10, 40, 4096)
_PARITY = {}   # (outliers, s, max_iteration) -> compared (False: left out for its margin)


def check_parity(s, max_iteration):
    for o in PARITY_OUTLIERS:
        if (o, s, max_iteration) in _PARITY:
            continue
        got, want, kept = check_run(dref.parity_problem(o, s), max_iteration)
        _PARITY[(o, s, max_iteration)] = kept
        print(f"s {s} outliers {o} max_iteration {max_iteration}: {want.n_iterations} iterations, {want.n_models} models, minNFA {want.min_nfa:.4g}, margin "
              f"{want.margin:.3g} ({want.margin_where}), {'compared' if kept else 'LEFT OUT'}")


def check_left_out_cap():
    """at most 5 % of the parity grid (one run of 36) may be left out for a margin below the guard (runs what test_loop_parity has not)"""
    for s in PARITY_S:
        for it in PARITY_ITERATIONS:
            check_parity(s, it)
    left_out = [k for k, kept in _PARITY.items() if not kept]
    print(f"left out: {len(left_out)} of {len(_PARITY)} {left_out}")
    assert len(_PARITY) == 36 and len(left_out) <= 0.05 * len(_PARITY)


def check_form_independence(outliers, s, max_iteration=4096):
    pr = dref.parity_problem(outliers, s)
    n = len(pr["x2d"])
    base, st0 = run_device([pr], max_iteration=max_iteration)
    for forms in (dict(waves_ahead=1), dict(waves_ahead=2), dict(waves_ahead=W), dict(global_above=n - 1), dict(global_above=n),
                  dict(global_above=n - 1, waves_ahead=3)):
        got, st = run_device([pr], max_iteration=max_iteration, **forms)
        assert same(got[0], base[0]) and st.n_iterations == st0.n_iterations and st.n_models == st0.n_models, f"form {forms} changes the result"
    check_self_consistent(pr, base[0])


def clean_problem(n, seed, noise=0.01):
    return ref.problem(n, ref.PINHOLE, 0.0, noise=noise, seed=seed)


def check_tiny():
    """n = 6: not ok, nothing written, 0 iterations; n = 7: the only k is 7"""
    got, stats = run_device([clean_problem(6, 1)])
    assert not got[0].ok and len(got[0].inliers) == 0 and got[0].error_max == 0.0 and got[0].min_nfa == 0.0 and stats.n_iterations == 0
    got, want, _ = check_run(clean_problem(7, 2), 64)
    assert not got.ok and len(got.inliers) in (0, 7) and len(want.inliers) in (0, 7)
    assert all(k == 7 for _, k, _ in got.better)


def check_fifteen_and_sixteen():
    """all points fit: fifteen inliers are too few (15 > 15 is false), sixteen are enough"""
    got15, _, _ = check_run(clean_problem(15, 3), 64)
    got16, _, _ = check_run(clean_problem(16, 4), 64)
    assert len(got15.inliers) == 15 and not got15.ok and got15.error_max < 0.1
    assert len(got16.inliers) == 16 and got16.ok and got16.error_max < 0.1


def check_size_edge(n):
    """lane-stride and sort-padding edges: 63, 64, 65, 128, 129 correspondences, in LDS and in global scratch, bit for bit the same"""
    pr = ref.problem(n, ref.PINHOLE, 0.3, seed=1000 + n)
    got, _, _ = check_run(pr, 40)
    assert got.ok and not pr["is_outlier"][got.inliers].any()
    other, _ = run_device([pr], max_iteration=40, global_above=n - 1)
    assert same(other[0], got)


def check_lds_threshold(max_iteration=10):
    """the largest problem of the LDS form, in LDS and (forced) in global scratch: the same bits; one more correspondence: global scratch
    by the host's own choice, with and without a (void) request for LDS"""
    pr = ref.problem(LDS_MAX_N, ref.PINHOLE, 0.3, seed=4321)
    a, sa = run_device([pr], max_iteration=max_iteration)
    b, sb = run_device([pr], max_iteration=max_iteration, global_above=LDS_MAX_N - 1)
    assert same(a[0], b[0]) and sa.n_models == sb.n_models and a[0].ok
    check_self_consistent(pr, a[0])
    pr = ref.problem(LDS_MAX_N + 1, ref.PINHOLE, 0.3, seed=4322)
    a, sa = run_device([pr], max_iteration=max_iteration)
    b, sb = run_device([pr], max_iteration=max_iteration, global_above=4 * LDS_MAX_N)
    assert same(a[0], b[0]) and sa.n_models == sb.n_models and a[0].ok
    check_self_consistent(pr, a[0])


def check_iteration_edge(max_iteration):
    """max_iteration = 1, 9 (no reserve), 10 (a reserve of one) and 4 096"""
    pr = ref.problem(50, ref.PINHOLE, 0.3, seed=77)
    got, want, kept = check_run(pr, max_iteration)
    assert kept and want.n_iterations <= max_iteration
    if max_iteration == 1:
        assert want.n_iterations == 1


def check_tied_residuals():
    """every correspondence twice: pairs of residuals equal to the bit, which order by index (std::pair<double, uint32_t>)"""
    half = ref.problem(24, ref.PINHOLE, 0.0, seed=34)
    pr = dict(half, x2d=np.concatenate([half["x2d"], half["x2d"]]), X3d=np.concatenate([half["X3d"], half["X3d"]]),
              is_outlier=np.concatenate([half["is_outlier"]] * 2))
    # the pool's first six draws of 48: a sample with a point and its copy has a rank-deficient design matrix and fails the ratio gate
    got, stats = run_device([pr], max_iteration=40, trace_events=TRACE_EVENTS)
    got = got[0]
    assert got.ok and len(got.inliers) >= 32
    pos = {int(v): i for i, v in enumerate(got.inliers)}
    pairs = [(i, i + 24) for i in range(24) if i in pos and i + 24 in pos]
    assert len(pairs) >= 16 and all(pos[b] == pos[a] + 1 for a, b in pairs)   # equal residuals: the lower index first, and at once
    want = dref.localize(pr["x2d"], pr["X3d"], WH, max_iteration=40, heads={it: head for it, _, head in got.better})
    if want.margin >= guard():
        compare(got, stats.n_iterations, stats.n_models, want)


def check_all_outliers():
    """nothing but uniform pixels: minNFA >= 0, the result is cleared"""
    pr = ref.problem(40, ref.PINHOLE, 1.0, seed=5)
    got, want, _ = check_run(pr, 40)
    assert want.min_nfa >= 0 and not want.ok and len(want.inliers) == 0
    assert got.min_nfa >= 0 and not got.ok and len(got.inliers) == 0


def check_coplanar():
    """every point on one plane: the design matrix has a two-dimensional null space, every sample fails the ratio gate, vec_inliers stays
    empty and the end-of-nIter branch extends the loop (++nIter; --nIterReserve) until the reserve is used up"""
    pr = ref.problem(20, ref.PINHOLE, 0.0, seed=6)
    rng = np.random.default_rng(7)
    pr["X3d"] = np.stack([rng.uniform(-2, 2, 20), rng.uniform(-2, 2, 20), np.full(20, 3.0)], 1)
    want = dref.localize(pr["x2d"], pr["X3d"], WH, max_iteration=40)
    assert ("extend" in [w for _, w in want.trace]) and want.n_models == 0 and want.n_iterations == 40 and "ratio rejected" in want.branches
    got, stats = run_device([pr], max_iteration=40)
    assert not got[0].ok and len(got[0].inliers) == 0 and stats.n_iterations == 40 and stats.n_models == 0
    assert got[0].min_nfa == np.inf and got[0].error_max == np.inf


def check_mixed_batch():
    """edges in one call, an empty problem in the middle, start with an offset into larger arrays, another image size per problem: each
    result is the single call's"""
    prs = [clean_problem(6, 1), ref.problem(65, ref.PINHOLE, 0.3, seed=1065), clean_problem(15, 3), None, ref.problem(40, ref.PINHOLE, 1.0, seed=5),
           dref.parity_problem(0.3, 2), clean_problem(16, 4), ref.problem(129, ref.PINHOLE, 0.3, seed=1129), dref.parity_problem(0.6, 3)]
    whs = [(1280 + 16 * i, 960 + 10 * i) for i in range(len(prs))]
    batch, stats = run_device(prs, offset=5, wh=whs, max_iteration=40, global_above=100)
    assert stats.n_problems == len(prs)
    total = 0
    for p, wh, b in zip(prs, whs, batch):
        if p is None:
            assert not b.ok and len(b.inliers) == 0
            continue
        single, st = run_device([p], wh=[wh], max_iteration=40, global_above=100)
        assert same(single[0], b)
        total += st.n_iterations
    assert stats.n_iterations == total
    other, _ = run_device([prs[1]], wh=[WH], max_iteration=40)
    assert not same(other[0], batch[1])   # the image size is read: it sets the normalisation


def check_arguments():
    pr = dref.parity_problem(0.3, 1)
    n = len(pr["x2d"])
    lib = _capi.lib()

    def call(start=(0, n), wh=(WH,), x2d=pr["x2d"], K=True, **kw):
        start = np.asarray(start, np.uint64)
        n_problems = len(start) - 1
        opt = resection.default_options(**dict(dict(solver=0), **kw))
        wh = None if wh is None else np.ascontiguousarray(wh, np.uint32)
        ok, pose, P, Kout = np.zeros(n_problems, np.uint8), np.zeros((n_problems, 15)), np.zeros((n_problems, 12)), np.zeros((n_problems, 9))
        err, nfa, inl_start, inl = np.zeros(n_problems), np.zeros(n_problems), np.zeros(n_problems + 1, np.uint64), np.zeros(1 << 17, np.uint32)
        import ctypes as C
        return lib.mvgx_resection_localize_uncalibrated(
            -1, n_problems, start.ctypes.data, None if x2d is None else x2d.ctypes.data, pr["X3d"].ctypes.data, None if wh is None else wh.ctypes.data,
            C.byref(opt), ok.ctypes.data, pose.ctypes.data, P.ctypes.data, Kout.ctypes.data if K else None, err.ctypes.data, nfa.ctypes.data,
            inl_start.ctypes.data, inl.ctypes.data, None)

    assert call(max_iteration=9) == _capi.MVGX_OK
    for solver in (1, 2, 3, 4, 5, -1):
        assert call(solver=solver) == _capi.MVGX_ERR_ARG
    assert call(error_max=4.0) == _capi.MVGX_ERR_UNSUPPORTED
    assert call(wh=((0, 960),)) == _capi.MVGX_ERR_ARG and call(wh=((1280, 0),)) == _capi.MVGX_ERR_ARG
    assert call(wh=None) == _capi.MVGX_ERR_ARG and call(x2d=None) == _capi.MVGX_ERR_ARG and call(K=False) == _capi.MVGX_ERR_ARG
    assert call(start=(0, n, n - 1), wh=(WH, WH)) == _capi.MVGX_ERR_ARG
    assert call(start=(0, 65537)) == _capi.MVGX_ERR_ARG
    assert call(waves_ahead=W + 1) == _capi.MVGX_ERR_ARG


def check_calibrated_entry_unchanged():
    """resection.localize(..., solver="dlt6") still has no device path: the uncalibrated problem is another entry's"""
    pr = dref.parity_problem(0.3, 1)
    try:
        resection.localize([0, len(pr["x2d"])], pr["x2d"], pr["X3d"], [pr["model"]], [pr["intr"]], solver="dlt6")
        code = _capi.MVGX_OK
    except _capi.MvgxError as e:
        code = e.code
    assert code == _capi.MVGX_ERR_UNSUPPORTED


def check_intrinsic_seed():
    """the intrinsics the engine would create: the restatement's to tolerance, and within 2 % of the generating (f, cx, cy) at 0.5 px noise
    on 60 points"""
    pr = dref.parity_problem(0.0, 0)   # 60 correspondences, no outliers
    assert len(pr["x2d"]) == 60
    got, want, kept = check_run(pr, 4096)
    assert kept and got.ok and len(got.inliers) >= 16
    seed, seed_want = np.array(resection.intrinsic_seed(got)), np.array(dref.intrinsic_seed(want.K))
    assert rel(seed, seed_want) <= loop_tol()[2]
    truth = pr["intr"][:3]
    print("intrinsic seed", seed, "generated with", truth)
    assert np.all(np.abs(seed / truth - 1.0) <= 0.02)
