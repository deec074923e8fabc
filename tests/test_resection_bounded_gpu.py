"""GPU: mvgx_resection_localize_bounded on the MI355X against the float64 restatement of the reference's bounded loop
(tests/_resection_bounded_ref.py). The cases are in tests/_resection_bounded_cases.py; the CPU twin (emulation) is
tests/test_resection_bounded_emu_cpu.py."""
import pytest

from tests import _resection_bounded_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("max_iteration", cases.PARITY_ITERATIONS)
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_loop_parity(built_lib, model, max_iteration):
    cases.check_parity(model, max_iteration)


def test_loop_parity_left_out_cap(built_lib):
    cases.check_left_out_cap()


@pytest.mark.parametrize("outliers", [0.0, 0.3])
@pytest.mark.parametrize("model", cases.PARITY_MODELS)
def test_form_independence(built_lib, model, outliers):
    cases.check_form_independence(model, outliers, 4096)


def test_form_independence_with_the_switch_inside_a_block(built_lib):
    cases.check_switch_mid_block()


def test_switch_threshold_seven_and_eight(built_lib):
    cases.check_switch_threshold()


@pytest.mark.parametrize("max_iteration", sorted(cases.EARLY_EXIT))
def test_early_exit_counts(built_lib, max_iteration):
    cases.check_early_exit(max_iteration)


def test_epsilon_gate(built_lib):
    cases.check_epsilon_gate()


@pytest.mark.parametrize("n", [4, 63, 64, 65, 511, 512, 513, cases.LDS_MAX_N, cases.LDS_MAX_N + 1])
def test_size_edges(built_lib, n):
    cases.check_size_edge(n)


def test_nordberg_loop(built_lib):
    cases.check_nordberg_loop()


def test_mixed_batch_with_offset(built_lib):
    cases.check_mixed_batch()


def test_arguments(built_lib):
    cases.check_arguments()
