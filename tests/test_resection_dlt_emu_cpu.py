"""CPU: mvgx_resection_localize_uncalibrated and the six-point solver - the device code of openmvg_amd/csrc/mvgx_resection_dlt.h under the
HIP emulation (tests/_emu.py) against the float64 restatement of the reference (tests/_resection_dlt_ref.py). The cases are in
tests/_resection_dlt_cases.py; the -m gpu twin of this file is tests/test_resection_dlt_gpu.py."""
import pytest

from tests import _emu
from tests import _resection_dlt_cases as cases


@pytest.fixture(autouse=True)
def _emulated():
    with _emu.emulated():
        yield


def test_solver_alone():
    cases.check_solver()


@pytest.mark.parametrize("max_iteration", cases.PARITY_ITERATIONS)
@pytest.mark.parametrize("s", cases.PARITY_S)
def test_loop_parity(s, max_iteration):
    cases.check_parity(s, max_iteration)


def test_loop_parity_left_out_cap():
    cases.check_left_out_cap()


@pytest.mark.parametrize("outliers", cases.PARITY_OUTLIERS)
def test_form_independence(outliers):
    cases.check_form_independence(outliers, 1, 200)   # (the -m gpu twin runs the whole grid's problems at 4 096 iterations)


def test_tiny_problems():
    cases.check_tiny()


def test_fifteen_and_sixteen_inliers():
    cases.check_fifteen_and_sixteen()


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_size_edges(n):
    cases.check_size_edge(n)


def test_lds_threshold():
    cases.check_lds_threshold(10)


@pytest.mark.parametrize("max_iteration", [1, 9, 10, 4096])
def test_iteration_edges(max_iteration):
    cases.check_iteration_edge(max_iteration)


def test_tied_residuals_order_by_index():
    cases.check_tied_residuals()


def test_all_outliers():
    cases.check_all_outliers()


def test_coplanar_points_extend_the_loop():
    cases.check_coplanar()


def test_mixed_batch_with_offset_and_image_sizes():
    cases.check_mixed_batch()


def test_arguments():
    cases.check_arguments()


def test_calibrated_entry_still_refuses_dlt6():
    cases.check_calibrated_entry_unchanged()


def test_intrinsic_seed():
    cases.check_intrinsic_seed()
