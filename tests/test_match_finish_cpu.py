"""The cases of tests/test_match_finish_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): the transposed finish of l2_filter16_kernel - which lane group ends up with which block of
the unit, the operand roles of the six merges, the norms a lane fetches at the start and the addresses it stores to - runs here with the
exchange in its shuffle-and-select form. What this cannot check is the lane-swap instructions themselves and gfx950 code generation."""
from tests import _emu, _match_finish_cases as cases


def test_inputs_cover_the_finish_cases():
    cases.inputs_cover_the_finish_cases()


def test_lists_equal_the_reference():
    with _emu.emulated():
        cases.check_lists()


def test_reused_slots_with_another_filter_in_between():
    with _emu.emulated():
        cases.check_reused_slots()
