"""GPU tests of the geometric filter's entries and launch forms at the edges of its size classes: for each of the six models one call with
pairs of m, 0, m + 1, 9, 64, 65, 256 and 257 correspondences (m = the minimal sample) - both sides of the boundary between the pairs whose
tables live in LDS and those whose tables live in global scratch. The indexed entry against the gathered one, MVGX_GEO_GLOBAL_ABOVE=8 and
(H, E) MVGX_GEO_AHEAD=1 against the default form: the same bytes, no tolerance. Inputs and checks live in tests/_geofilter_entry_cases.py,
shared with the CPU run of the same source (tests/test_geofilter_entry_cpu.py)."""
import pytest

from tests import _geofilter_entry_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", cases.MODELS)
def test_indexed_entry_equals_the_gathered_entry(model):
    cases.check_indexed_equals_gathered(model, 257, emulated=False)


@pytest.mark.parametrize("model", cases.MODELS)
def test_global_table_form_equals_the_default_form(model):
    cases.check_global_form_equals_default(model, 257, emulated=False)


@pytest.mark.parametrize("model", ["h", "e"])
def test_one_sample_per_iteration_equals_samples_ahead(model):
    cases.check_one_sample_per_iteration_equals_default(model, 257, emulated=False)


@pytest.mark.parametrize("model", cases.MODELS)
def test_pairs_of_at_most_a_minimal_sample_are_rejected(model):
    cases.check_small_pairs_are_rejected(model, 257, emulated=False)
