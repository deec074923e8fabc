"""GPU tests of the dense query layout of the default matching filter: l2_filter16_kernel reads its query fragments from tiles that keep
an image's rows in their original order (ceil(n / 32) per image), while the database side keeps the tiles split by norm parity; the verify
stage, the candidate count and the compaction read a query slot of that filter's output as the original row. Offsets and (i, j) lists are
integers: they are compared for equality with the reference, no tolerance. Inputs and checks live in tests/_match_dense_cases.py (shared
with the CPU run of the same device source, tests/test_matching_dense_query_cpu.py)."""
import pytest

from tests import _match_dense_cases as cases

pytestmark = pytest.mark.gpu


def test_cases_are_what_they_claim():
    cases.check_cases_are_what_they_claim()


@pytest.mark.parametrize("kind", ["sorted", "both"])
def test_default_filter_equals_reference(kind):
    cases.check_default_equals_reference(kind)


@pytest.mark.parametrize("batch_pairs", [2, 5])
def test_batch_seams_and_reused_slots(batch_pairs):
    cases.check_batch_seams(batch_pairs)


def test_parity_slot_filters_agree_and_layouts_alternate_on_one_context():
    cases.check_cross_check_shapes()


def test_every_option_combination_resolves_to_a_form_that_equals_the_reference():
    cases.check_form_resolution(cases.FORMS_ALL)


def test_debug_filter_accepts_the_three_epilogue_forms_only():
    cases.check_debug_filter_values()


def test_unknown_filter_form_in_the_environment_is_ignored(monkeypatch):
    monkeypatch.setenv("MVGX_MATCH_FILTER", "3")
    cases.check_env_filter_ignored()
