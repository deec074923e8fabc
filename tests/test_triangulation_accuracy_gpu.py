"""GPU: the points of mvgx_triangulate_tracks on the MI355X against 50-digit solutions on hard geometry - scenes away from the origin and
small parallax (tests/_triangulation_accuracy_cases.py has the families and the rule; tests/golden/triangulation_truth.npz the data).
Each test is one call on 100 tracks. The CPU twin (emulation) is tests/test_triangulation_accuracy_emu_cpu.py."""
import pytest

from tests import _triangulation_accuracy_cases as acc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", acc.FAMILIES)
@pytest.mark.parametrize("name,views,solver,kw", acc.CALLS, ids=acc.CALL_IDS)
def test_points_against_50_digits(built_lib, family, name, views, solver, kw):
    acc.check(family, name, views, solver, kw)
