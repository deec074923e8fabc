"""GPU tests of the wave-packed work list of the default matching filter: l2_filter16_kernel takes units of four query tiles, one per wave,
packed four to a workgroup across the pairs that share the database image, and the verify stage walks the same units. Offsets and (i, j)
lists are integers: they are compared for equality with the C restatement of the reference, no tolerance. Inputs and checks live in
tests/_match_wave_cases.py (shared with the CPU run of the same device source, tests/test_match_wave_packing_cpu.py); every run also
requires the context's error flag to be zero (MatchContext.run raises otherwise: see there)."""
import pytest

from tests import _match_wave_cases as cases
from tests.test_matching_gpu import run_hip

pytestmark = pytest.mark.gpu


def test_unit_counts_cover_every_remainder():
    cases.unit_counts_cover_every_remainder()


@pytest.mark.parametrize("kind", ["sorted", "both", "shuffled"])
def test_pair_order_never_mixes_database_images(kind):
    cases.check_pair_order(kind, run_hip)


@pytest.mark.parametrize("batch_pairs", [3, 8])
def test_batch_boundaries_and_reused_slots(batch_pairs):
    cases.check_batch_boundaries(batch_pairs)


def test_candidate_count_covers_exactly_the_written_units():
    cases.check_candidate_count()
