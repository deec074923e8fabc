"""CPU: the float64 restatement of the resection without intrinsics (tests/_resection_dlt_ref.py) against the compiled reference's
SixPointResectionSolver and ACRANSAC through ACKernelAdaptorResection, recorded in tests/golden/resection_dlt_golden.npz
(tests/golden/make_resection_dlt_golden.py): the yardstick of the device tests is itself pinned."""
import numpy as np
import pytest

from tests import _resection_dlt_cases as cases
from tests import _resection_dlt_ref as dref
from tests import _resection_ref as ref


def test_solver_restatement_against_the_reference():
    g = cases.gold()
    x, X = g["x_norm"], g["X"]
    tol_P, tol_ratio = cases.solver_tol()
    hit, worst, worst_ratio, decided = set(), 0.0, 0.0, 0
    for i in range(len(x)):
        mg = ref.Margin()
        models, ratio = dref.six_point(x[i], X[i], mg, hit)
        if mg.value >= cases.guard():
            decided += 1
            assert len(models) == g["ref_count"][i], f"sample {i}: number of models"
        worst_ratio = max(worst_ratio, abs(ratio / g["ref_ratio"][i] - 1.0))
        if models and g["ref_count"][i]:
            worst = max(worst, cases.rel(models[0], g["ref_P"][i]))
            assert np.array_equal(models[0], g["own_P"][i])   # the fixture's record of this restatement
    print(f"restatement against the reference: relative |dP| {worst:.3g}, ratio {worst_ratio:.3g}; {decided} of {len(x)} samples decided")
    assert worst <= tol_P and worst_ratio <= tol_ratio and decided >= 0.95 * len(x)
    assert cases.NEEDED_BRANCHES <= hit
    assert len(x) >= 400 and np.sum(g["group"] == 0) == 400


@pytest.mark.parametrize("max_iteration", cases.PARITY_ITERATIONS)
def test_loop_restatement_against_the_reference(max_iteration):
    g = cases.gold()
    tol_nfa, tol_err, tol_P = cases.loop_tol()
    at = np.concatenate([[0], np.cumsum(g["loop_n_inliers"])])
    runs = [i for i, row in enumerate(g["loop_grid"]) if int(row[2]) == max_iteration]
    assert len(runs) == 9 and len(g["loop_grid"]) == 36
    for i in runs:
        o, s = float(g["loop_grid"][i][0]), int(g["loop_grid"][i][1])
        pr = dref.parity_problem(o, s)
        own = dref.localize(pr["x2d"], pr["X3d"], max_iteration=max_iteration)
        inl = g["loop_inliers"][at[i]:at[i + 1]]
        if own.margin < cases.guard():
            continue   # (the fixture's generator holds these to one run of the 36)
        assert np.array_equal(own.inliers, inl), f"run {i}: inlier list (order included)"
        assert own.min_nfa == g["loop_min_nfa"][i] or abs(own.min_nfa - g["loop_min_nfa"][i]) <= tol_nfa * max(1.0, abs(g["loop_min_nfa"][i]))
        assert own.error_max == g["loop_error_max"][i] or abs(own.error_max - g["loop_error_max"][i]) <= tol_err * abs(g["loop_error_max"][i])
        if own.ok:
            assert cases.rel(own.P, g["loop_P"][i]) <= tol_P
        assert own.n_iterations == g["own_n_iterations"][i]


def test_left_out_cap_of_the_fixture():
    g = cases.gold()
    assert int((~g["loop_same"]).sum()) <= 0.05 * len(g["loop_same"])


def test_normalizer_goes_through_the_float_product():
    d, ox, oy = dref.normalizer(1280, 960)
    assert d == 1.0 / np.sqrt(1280.0 * 960.0) and ox == -640.0 * d and oy == -480.0 * d
    w = (1 << 24) + 1   # the float product -.5f * width rounds here
    assert dref.normalizer(w, 1)[1] != -0.5 * w * dref.normalizer(w, 1)[0]
