"""GPU tests of the block-granular work list of the default matching filter: a wave of l2_filter16_kernel takes 8 consecutive blocks of 16
query rows from the block stream of the pairs that share the database image, running on from one query image into the next, and the
verify stage walks the same units. Offsets and (i, j) lists are integers: they are compared for equality with the C restatement of the
reference, no tolerance. Inputs and checks live in tests/_match_block_cases.py (shared with the CPU run of the same device source,
tests/test_match_block_units_cpu.py); every run also requires the context's error flag to be zero (MatchContext.run raises otherwise)."""
import pytest

from tests import _match_block_cases as cases

pytestmark = pytest.mark.gpu


def test_inputs_cover_the_packing_cases():
    cases.inputs_cover_the_packing_cases()


@pytest.mark.parametrize("kind", ["sorted", "both", "shuffled"])
def test_pair_order_never_mixes_database_images(kind):
    cases.check_pair_order(kind)


@pytest.mark.parametrize("batch_pairs", [3, 8])
def test_batch_boundaries_and_reused_slots(batch_pairs):
    cases.check_batch_boundaries(batch_pairs)


def test_mixed_filters_on_one_context():
    cases.check_mixed_filters()


def test_candidate_count_covers_exactly_the_written_blocks():
    cases.check_candidate_count()
