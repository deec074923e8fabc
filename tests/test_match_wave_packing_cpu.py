"""The cases of tests/test_match_wave_packing_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): the batch builder, the record format, the verify stage's read range and the kernel's
per-wave addressing are checked where no GPU exists. What this cannot check is gfx950 code generation and timing."""
import pytest

from tests import _emu, _match_wave_cases as cases
from tests.test_matching_gpu import run_hip


def test_unit_counts_cover_every_remainder():
    cases.unit_counts_cover_every_remainder()


@pytest.mark.parametrize("kind", ["sorted", "both", "shuffled"])
def test_pair_order_never_mixes_database_images(kind):
    with _emu.emulated():
        cases.check_pair_order(kind, run_hip)


@pytest.mark.parametrize("batch_pairs", [3, 8])
def test_batch_boundaries_and_reused_slots(batch_pairs):
    with _emu.emulated():
        cases.check_batch_boundaries(batch_pairs)


def test_candidate_count_covers_exactly_the_written_units():
    with _emu.emulated():
        cases.check_candidate_count()
