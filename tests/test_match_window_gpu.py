"""GPU tests of the window structure of the default matching filter (l2_filter16_kernel): a full window of 8 tiles runs unrolled with its
first tile peeled, the short window of an image keeps the tile loop, the window maxima are folded into a running top-2 once per window.
Database images of 1, 7, 8, 9, 16 and 17 tiles (and one of natural norm parity) with planted best rows and runner-ups in every place where
the paths differ; the (i, j) lists are integers and are compared entry by entry with the compiled reference (its C restatement where that
is not built), no tolerance. Inputs and checks live in tests/_match_window_cases.py, shared with the CPU run of the same device source
(tests/test_match_window_cpu.py)."""
import pytest

from tests import _match_window_cases as cases

pytestmark = pytest.mark.gpu


def test_cases_are_what_they_claim():
    cases.check_cases_are_what_they_claim()


def test_lists_equal_the_reference_in_every_window_shape():
    cases.check_lists()
