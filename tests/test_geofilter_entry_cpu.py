"""The cases of tests/test_geofilter_entry_gpu.py under the HIP execution-model emulation (tests/_emu.py compiles
openmvg_amd/csrc/mvgx_geofilter.hip for the host): the ten entries, the two table forms and the two sample forms return the same bytes
where no GPU exists. One fiber per lane makes large pairs slow: every model runs the sizes up to 65 (the global-table form forced by
MVGX_GEO_GLOBAL_ABOVE=8), the fundamental model also 256 and 257 - the two sides of the real LDS / global boundary."""
import pytest

from tests import _geofilter_entry_cases as cases

CASES = [(m, 65) for m in cases.MODELS] + [("f", 257)]


@pytest.mark.parametrize("model,limit", CASES)
def test_indexed_entry_equals_the_gathered_entry(model, limit):
    cases.check_indexed_equals_gathered(model, limit, emulated=True)


@pytest.mark.parametrize("model,limit", CASES)
def test_global_table_form_equals_the_default_form(model, limit):
    cases.check_global_form_equals_default(model, limit, emulated=True)


@pytest.mark.parametrize("model", ["h", "e"])
def test_one_sample_per_iteration_equals_samples_ahead(model):
    cases.check_one_sample_per_iteration_equals_default(model, 65, emulated=True)


@pytest.mark.parametrize("model,limit", CASES)
def test_pairs_of_at_most_a_minimal_sample_are_rejected(model, limit):
    cases.check_small_pairs_are_rejected(model, limit, emulated=True)
