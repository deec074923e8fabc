"""The cases of tests/test_matching_dense_query_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_match.hip for the host): the dense tile build, the batch builder, the filter's query addressing and the slot
numbering that the verify stage, the candidate count and the compaction read are checked where no GPU exists. What this cannot check is
gfx950 code generation and timing. The emulation is slow: the multi-run checks take the exhaustive pair list without its mirror (78
pairs; the mirrored list runs once, in test_default_filter_equals_reference)."""
import pytest

from tests import _emu, _match_dense_cases as cases


def test_cases_are_what_they_claim():
    cases.check_cases_are_what_they_claim()


@pytest.mark.parametrize("kind", ["sorted", "both"])
def test_default_filter_equals_reference(kind):
    with _emu.emulated():
        cases.check_default_equals_reference(kind)


@pytest.mark.parametrize("batch_pairs", [2, 5])
def test_batch_seams_and_reused_slots(batch_pairs):
    with _emu.emulated():
        cases.check_batch_seams(batch_pairs, "sorted")


def test_parity_slot_filters_agree_and_layouts_alternate_on_one_context():
    with _emu.emulated():
        cases.check_cross_check_shapes("sorted")


def test_option_combinations_no_other_test_reaches_resolve_to_forms_that_equal_the_reference():
    with _emu.emulated():
        cases.check_form_resolution(cases.FORMS_UNREACHED)


def test_debug_filter_accepts_the_three_epilogue_forms_only():
    with _emu.emulated():
        cases.check_debug_filter_values()


def test_unknown_filter_form_in_the_environment_is_ignored(monkeypatch):
    monkeypatch.setenv("MVGX_MATCH_FILTER", "3")
    with _emu.emulated():
        cases.check_env_filter_ignored()
