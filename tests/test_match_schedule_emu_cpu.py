"""The cases of tests/test_match_schedule_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): a run that starts and ends on small batches ("batch_ramp") and the record order inside an
XCD's slice ("record_order") leave every list as it was, on one context and on two that share the batches of a run. What this cannot
check is timing - the point of both - and gfx950 code generation. The one-batch case of the GPU test stays there: the ramped runs' batches
already hold several database images per slice, and 780 pairs twice take the emulation a quarter of a minute."""
import pytest

from tests import _emu, _match_schedule_cases as cases


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_ramped_run_equals_the_reference(devices):
    """(both record orders in one case: the first collecting run has the order off, everything after it on)"""
    with _emu.emulated():
        cases.check_ramped_run(devices, 1)
