"""The cases of tests/test_match_window_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): the peeled first tile of a window, the unrolled full window and the short one, the fold of
the window maxima and the finish are checked where no GPU exists. What this cannot check is gfx950 code generation, the staging
statements (the emulation copies per lane) and timing."""
from tests import _emu, _match_window_cases as cases


def test_cases_are_what_they_claim():
    cases.check_cases_are_what_they_claim()


def test_lists_equal_the_reference_in_every_window_shape():
    with _emu.emulated():
        cases.check_lists()
