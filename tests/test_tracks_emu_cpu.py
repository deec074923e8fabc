"""CPU: mvgx_tracks_build - the device code of openmvg_amd/csrc/mvgx_tracks.h under the HIP emulation (tests/_emu.py) against the compiled
reference's outputs (tests/golden/tracks_golden.npz) and the restatement (tests/_tracks_ref.py). The cases are in tests/_tracks_cases.py;
the -m gpu twin of this file is tests/test_tracks_gpu.py. The emulation runs the workgroups of a launch one after the other, so the
labelling needs two sweeps here whatever the graph; the collision case runs at the header's capacity."""
import pytest

from tests import _emu
from tests import _tracks_cases as cases


@pytest.fixture(autouse=True)
def _emulated():
    with _emu.emulated():
        yield


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
    cases.check_long_path(257)


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
