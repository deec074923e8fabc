"""GPU: mvgx_tracks_build on the MI355X against the compiled reference's outputs (tests/golden/tracks_golden.npz) and the restatement
(tests/_tracks_ref.py). The cases are in tests/_tracks_cases.py; the CPU twin (emulation) is tests/test_tracks_emu_cpu.py."""
import pytest

from tests import _tracks_cases as cases

pytestmark = pytest.mark.gpu


def test_edges_of_nothing():
    cases.check_nothing()


def test_fixture_cases():
    cases.check_fixture()


def test_mask_equals_compacted_lists():
    cases.check_mask()


@pytest.mark.parametrize("n", cases.EDGE_SIZES)
@pytest.mark.parametrize("kind", ["matches", "nodes"])
def test_lane_and_workgroup_edges(kind, n):
    cases.check_edge(kind, n)


def test_long_component():
    print("long path of 4097 nodes: n_sweeps", cases.check_long_path(4097))


def test_collision_forms():
    cases.check_collision_forms()


def test_track_as_long_as_the_image_count():
    cases.check_full_length_track()


def test_reproducible():
    cases.check_reproducible()


def test_arguments():
    cases.check_arguments()


def test_handover_to_triangulation():
    cases.check_handover()
