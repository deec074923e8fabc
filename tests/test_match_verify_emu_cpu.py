"""The cases of tests/test_match_verify_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): the candidate ranking of a unit, the transposed reduction, the norms from the tables, the
valid mask of the cell and the two pairs of a unit are checked where no GPU exists. The lane scatter / gather and the first dot product of
a row have a host form in the source (as the window staging has); gfx950 code generation and timing are not checked here."""
from tests import _emu, _match_verify_cases as cases


def test_inputs_are_what_they_claim():
    cases.inputs_are_what_they_claim()


def test_lists_equal_the_reference_and_candidates_are_the_planted_ones():
    with _emu.emulated():
        cases.check_lists_and_candidates()


def test_repeated_runs_with_the_other_verify_form_between_them():
    with _emu.emulated():
        cases.check_repeated_and_interleaved()
