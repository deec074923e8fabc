"""GPU: mvgx_resection_localize and the P3P solvers on the MI355X against the float64 restatement of the reference
(tests/_resection_ref.py). The cases are in tests/_resection_cases.py; the CPU twin (emulation) is tests/test_resection_emu_cpu.py."""
import numpy as np
import pytest

from tests import _resection_cases as cases
from tests import _resection_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("solver", ["ding", "nordberg"])
def test_solver_alone(built_lib, solver):
    cases.check_solver(solver)


@pytest.mark.parametrize("max_iteration", cases.PARITY_ITERATIONS)
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_loop_parity(built_lib, model, max_iteration):
    cases.check_parity(model, max_iteration)


def test_loop_parity_left_out_cap(built_lib):
    cases.check_left_out_cap()


@pytest.mark.parametrize("outliers", cases.PARITY_OUTLIERS)
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_form_independence(built_lib, model, outliers):
    cases.check_form_independence(model, outliers, 4096)


def test_tiny_problems(built_lib):
    cases.check_tiny()


def test_seven_and_eight_inliers(built_lib):
    cases.check_seven_and_eight()


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_size_edges(built_lib, n):
    cases.check_size_edge(n)


@pytest.mark.parametrize("max_iteration", [1, 9, 10, 4096])
def test_iteration_edges(built_lib, max_iteration):
    cases.check_iteration_edge(max_iteration)


def test_tied_residuals_order_by_index(built_lib):
    cases.check_tied_residuals()


def test_all_outliers(built_lib):
    cases.check_all_outliers()


def test_no_model_at_all_extends_the_loop(built_lib):
    cases.check_no_model_at_all()


def test_mixed_batch_with_offset(built_lib):
    cases.check_mixed_batch()


def test_arguments(built_lib):
    cases.check_arguments()


def test_nordberg_loop(built_lib):
    cases.check_nordberg_loop()


def test_pose_row_feeds_the_ba_scene(built_lib):
    cases.check_pose_row()


def test_storage_threshold(built_lib):
    """1 024 correspondences (the largest problem of the LDS form), 1 025 (global scratch) and both with the other form forced: real
    waves, the whole LDS budget, the same bits"""
    for n in (1024, 1025):
        pr = ref.problem(n, ref.PINHOLE, 0.3, seed=n)
        got, st = cases.run_device([pr], max_iteration=200)
        other, st2 = cases.run_device([pr], max_iteration=200, global_above=512, waves_ahead=3)
        assert cases.same(got[0], other[0]) and st.n_iterations == st2.n_iterations
        cases.check_self_consistent(pr, got[0])
        assert got[0].ok and not pr["is_outlier"][got[0].inliers].any()
        assert np.abs(got[0].R - pr["R"]).max() < 5e-3
