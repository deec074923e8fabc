"""GPU tests of the verify stage behind the default matching filter (l2_verify_kernel<true>): candidates per 64-slot part from none to all,
ranks that run from part 0 into part 1 and past 63, units of two pairs, database images from 1 to 530 rows and one with three rows in
its odd half, runner-ups inside the winner's cell on both sides of the fp32 ratio test and ties. Offsets and (i, j) lists are integers:
they are compared entry by entry with the compiled reference (oracle/_ref), no tolerance. Inputs and checks live in
tests/_match_verify_cases.py (shared with the CPU run of the same device source, tests/test_match_verify_emu_cpu.py); every run also
requires the context's error flag to be zero (MatchContext.run raises otherwise)."""
import pytest

from tests import _match_verify_cases as cases

pytestmark = pytest.mark.gpu


def test_inputs_are_what_they_claim():
    cases.inputs_are_what_they_claim()


def test_lists_equal_the_reference_and_candidates_are_the_planted_ones():
    cases.check_lists_and_candidates()


def test_repeated_runs_with_the_other_verify_form_between_them():
    cases.check_repeated_and_interleaved()
