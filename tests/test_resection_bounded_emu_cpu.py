"""CPU: mvgx_resection_localize_bounded - the device code of openmvg_amd/csrc/mvgx_resection.h under the HIP emulation (tests/_emu.py)
against the float64 restatement of the reference's bounded loop (tests/_resection_bounded_ref.py). The cases are in
tests/_resection_bounded_cases.py; the -m gpu twin of this file is tests/test_resection_bounded_gpu.py."""
import pytest

from tests import _emu
from tests import _resection_bounded_cases as cases


@pytest.fixture(autouse=True)
def _emulated():
    with _emu.emulated():
        yield


@pytest.mark.parametrize("max_iteration", cases.PARITY_ITERATIONS)
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_loop_parity(model, max_iteration):
    cases.check_parity(model, max_iteration)


def test_loop_parity_left_out_cap():
    cases.check_left_out_cap()


@pytest.mark.parametrize("outliers", [0.0, 0.3])
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_form_independence(model, outliers):
    cases.check_form_independence(model, outliers, 200)   # (the -m gpu twin runs the same problems at 4 096 iterations)


def test_form_independence_with_the_switch_inside_a_block():
    cases.check_switch_mid_block()


def test_switch_threshold_seven_and_eight():
    cases.check_switch_threshold()


@pytest.mark.parametrize("max_iteration", sorted(cases.EARLY_EXIT))
def test_early_exit_counts(max_iteration):
    cases.check_early_exit(max_iteration)


def test_epsilon_gate():
    cases.check_epsilon_gate()


@pytest.mark.parametrize("n", [4, 63, 64, 65, 511, 512, 513, cases.LDS_MAX_N, cases.LDS_MAX_N + 1])
def test_size_edges(n):
    cases.check_size_edge(n)


def test_nordberg_loop():
    cases.check_nordberg_loop()


def test_mixed_batch_with_offset():
    cases.check_mixed_batch()


def test_arguments():
    cases.check_arguments()
