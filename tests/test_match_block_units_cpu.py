"""The cases of tests/test_match_block_units_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): the record builder, the per-block selection of a wave's query fragments, results and store
addresses, and the verify stage's walk over the same units are checked where no GPU exists. What this cannot check is gfx950 code
generation and timing."""
import pytest

from tests import _emu, _match_block_cases as cases


def test_inputs_cover_the_packing_cases():
    cases.inputs_cover_the_packing_cases()


@pytest.mark.parametrize("kind", ["sorted", "both", "shuffled"])
def test_pair_order_never_mixes_database_images(kind):
    with _emu.emulated():
        cases.check_pair_order(kind)


@pytest.mark.parametrize("batch_pairs", [3, 8])
def test_batch_boundaries_and_reused_slots(batch_pairs):
    with _emu.emulated():
        cases.check_batch_boundaries(batch_pairs)


def test_mixed_filters_on_one_context():
    with _emu.emulated():
        cases.check_mixed_filters()


def test_candidate_count_covers_exactly_the_written_blocks():
    with _emu.emulated():
        cases.check_candidate_count()
