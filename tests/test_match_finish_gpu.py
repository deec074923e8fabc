"""GPU tests of the transposed finish of the default matching filter (l2_filter16_kernel): after the last window the lane
groups of a wave swap halves of their eight per-block results (v_permlane16_swap_b32, v_permlane32_swap_b32), each group merges and
stores the two blocks it owns. Offsets and (i, j) lists are integers: they are compared for equality with the C restatement of the
reference, no tolerance. Inputs and checks live in tests/_match_finish_cases.py (shared with the CPU run of the same device source,
tests/test_match_finish_cpu.py): every (block of a unit, lane group of the best row) and every ordered (group of the best row, group of
the runner-up) among the accepted matches, ties for the first place across lane groups g and g ^ 2, every unit split, short last blocks
and blocks past the rows under every owner. Every run also requires the context's error flag to be zero (MatchContext.run raises)."""
import pytest

from tests import _match_finish_cases as cases

pytestmark = pytest.mark.gpu


def test_inputs_cover_the_finish_cases():
    cases.inputs_cover_the_finish_cases()


def test_lists_equal_the_reference():
    cases.check_lists()


def test_reused_slots_with_another_filter_in_between():
    cases.check_reused_slots()
