"""GPU tests of the batch schedule of a matching run and of the record order inside an XCD's slice: a run that starts and ends on small
batches (option "batch_ramp") hands over exactly the batches mvgx_match_batch_schedule tells, reuses slot buffers that were sized on a
small first batch, and returns the lists of the reference; so does the filter when the records of a slice are ordered by query chunk
(option "record_order"), with several database images in every slice. Offsets and (i, j) lists are integers: compared for equality with
the C restatement of the reference, no tolerance. Inputs and checks live in tests/_match_schedule_cases.py (shared with the CPU run of
the same source, tests/test_match_schedule_emu_cpu.py)."""
import pytest

from tests import _match_schedule_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("record_order", [0, 1])
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_ramped_run_equals_the_reference(devices, record_order):
    cases.check_ramped_run(devices, record_order)


def test_one_batch_with_several_database_images_per_slice():
    counts = {order: cases.check_one_batch_slices_of_several_database_images(order) for order in (0, 1)}
    assert counts[0] == counts[1] > 0, counts
