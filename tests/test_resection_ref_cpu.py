"""CPU: the float64 restatement of the robust resection (tests/_resection_ref.py) against what the compiled reference returned
(tests/golden/resection_golden.npz, written by tests/golden/make_resection_golden.py) and against the generating poses."""
import numpy as np
import pytest

from tests import _resection_cases as cases
from tests import _resection_ref as ref


@pytest.mark.parametrize("solver", ["ding", "nordberg"])
def test_restatement_reproduces_the_recorded_reference(solver):
    g = cases.gold()
    s = cases.SOLVER_INDEX[solver]
    worst = 0.0
    for i in range(len(g["X"])):
        models = ref.SOLVERS[solver](g["bearings"][i], g["X"][i])
        assert len(models) == g["ref_count"][s, i]
        for m, M in enumerate(models):
            worst = max(worst, float(np.abs(M - g["ref_Rt"][s, i, m]).max()))
            assert np.array_equal(M, g["own_Rt"][s, i, m])   # the restatement's own recorded output, bit for bit
    assert worst <= 10.0 * g["solver_spread"][s]


@pytest.mark.parametrize("solver", ["ding", "nordberg"])
def test_one_model_is_the_generating_pose(solver):
    B, X, R, t = ref.p3p_samples(50, seed=3)
    for i in range(len(B)):
        models = ref.SOLVERS[solver](B[i], X[i])
        assert min(np.abs(M - np.c_[R[i], t[i]]).max() for M in models) < 1e-8


def test_restatement_reproduces_the_recorded_reference_loop():
    """the reference's ACRANSAC on the parity grid: where the fixture says both returned the same inlier list they still do, with
    minNFA, threshold and P within 10 x the recorded spread; at least 27 of the 36 runs are such"""
    g = cases.gold()
    at = np.concatenate([[0], np.cumsum(g["loop_n_inliers"])])
    nfa_s, err_s, P_s = (10.0 * max(float(v), 1e-16) for v in g["loop_spread"])
    assert int(g["loop_same"].sum()) >= 27 and len(g["loop_grid"]) == 36
    for r, (m, o, it) in enumerate(g["loop_grid"]):
        if not g["loop_same"][r]:
            continue
        pr = cases.parity_problem(int(m), float(o))
        own = ref.localize(int(m), pr["intr"], pr["x2d"], pr["X3d"], max_iteration=int(it))
        assert np.array_equal(own.inliers, g["loop_inliers"][at[r]:at[r + 1]])
        assert abs(own.min_nfa - g["loop_min_nfa"][r]) <= nfa_s * max(1.0, abs(g["loop_min_nfa"][r]))
        if len(own.inliers):
            assert abs(own.error_max - g["loop_error_max"][r]) <= err_s * g["loop_error_max"][r]
        if own.ok:
            assert np.abs(own.P - g["loop_P"][r]).max() <= P_s


def test_krt_from_p_returns_a_rotation():
    rng = np.random.default_rng(0)
    for _ in range(20):
        pr = ref.problem(4, seed=int(rng.integers(1 << 30)))
        P = np.c_[pr["R"], pr["t"]] + rng.normal(size=(3, 4)) * 1e-13
        K, R, t = ref.krt_from_p(P)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0
        assert np.abs(K - np.eye(3)).max() < 1e-12 and np.abs(R - pr["R"]).max() < 1e-12 and np.abs(t - pr["t"]).max() < 1e-11


def test_loop_finds_the_pose_and_reports_when_it_stops_being_decided():
    pr = ref.problem(80, ref.PINHOLE, 0.3, seed=11)
    run = ref.localize(pr["model"], pr["intr"], pr["x2d"], pr["X3d"], max_iteration=4096)
    assert run.ok and not pr["is_outlier"][run.inliers].any() and np.abs(run.R - pr["R"]).max() < 5e-3
    assert run.n_iterations < 4096 and ("pool" in [w for _, w in run.trace])
    assert run.undecided_at is not None   # at full length a point of some adopted sample is drawn again
    short = ref.localize(pr["model"], pr["intr"], pr["x2d"], pr["X3d"], max_iteration=10)
    assert short.n_iterations <= 10 and short.margin > 0


def test_k_scan_keeps_the_lowest_k_among_equal_nfa():
    """strict <: the only NFA values that tie to the bit are infinities (non-finite residuals); the first of them is kept, and an
    infinite NFA never beats minNFA. (Two k with the same finite NFA do not occur: with <= for < the device passes every test.)"""
    zeros = np.zeros(9, np.float32)
    _, _, nfa = ref.nfa_scan(np.full(8, np.inf), 0.25, zeros, zeros)
    assert np.all(np.isinf(nfa)) and int(np.argmin(nfa)) == 0 and not (nfa[0] < np.inf)
    _, _, nfa = ref.nfa_scan(np.array([0.0, 0.0, 0.0, 0.0, 1e-6, np.inf, np.inf, np.inf]), 0.25, zeros, zeros)
    assert np.all(np.isinf(nfa[2:])) and int(np.argmin(nfa)) in (0, 1)


def test_sorted_ties_order_by_index():
    """equal residuals order by index (std::pair<double, uint32_t>): a hand-made tie"""
    e = np.array([0.5, 0.25, 0.5, 0.125, 0.25, np.nan])
    e[~np.isfinite(e)] = np.inf
    logc_n, logc_k = ref.logc_tables(len(e))
    order, r, nfa = ref.nfa_scan(e, 0.3, logc_n, logc_k)
    assert list(order) == [3, 1, 4, 0, 2, 5] and len(nfa) == 3
