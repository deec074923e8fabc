"""CPU: mvgx_resection_localize and the P3P solvers - the device code of openmvg_amd/csrc/mvgx_resection.h under the HIP emulation
(tests/_emu.py) against the float64 restatement of the reference (tests/_resection_ref.py). The cases are in tests/_resection_cases.py;
the -m gpu twin of this file is tests/test_resection_gpu.py."""
import pytest

from tests import _emu
from tests import _resection_cases as cases


@pytest.fixture(autouse=True)
def _emulated():
    with _emu.emulated():
        yield


@pytest.mark.parametrize("solver", ["ding", "nordberg"])
def test_solver_alone(solver):
    cases.check_solver(solver)


@pytest.mark.parametrize("max_iteration", cases.PARITY_ITERATIONS)
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_loop_parity(model, max_iteration):
    cases.check_parity(model, max_iteration)


def test_loop_parity_left_out_cap():
    cases.check_left_out_cap()


@pytest.mark.parametrize("outliers", cases.PARITY_OUTLIERS)
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_form_independence(model, outliers):
    cases.check_form_independence(model, outliers, 200)   # (the -m gpu twin runs the same problems at 4 096 iterations)


def test_tiny_problems():
    cases.check_tiny()


def test_seven_and_eight_inliers():
    cases.check_seven_and_eight()


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_size_edges(n):
    cases.check_size_edge(n)


@pytest.mark.parametrize("max_iteration", [1, 9, 10, 4096])
def test_iteration_edges(max_iteration):
    cases.check_iteration_edge(max_iteration)


def test_tied_residuals_order_by_index():
    cases.check_tied_residuals()


def test_all_outliers():
    cases.check_all_outliers()


def test_no_model_at_all_extends_the_loop():
    cases.check_no_model_at_all()


def test_mixed_batch_with_offset():
    cases.check_mixed_batch()


def test_arguments():
    cases.check_arguments()


def test_nordberg_loop():
    cases.check_nordberg_loop()


def test_pose_row_feeds_the_ba_scene():
    cases.check_pose_row()
