"""CPU, no library: the restatement of tracks::TracksBuilder (tests/_tracks_ref.py) against the compiled reference's outputs in
tests/golden/tracks_golden.npz, and what the fixture has to hold for the device tests to tell a wrong implementation from a right one."""
import os

import numpy as np

from tests import _tracks_ref as tref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_PATH = os.path.join(HERE, "golden", "tracks_golden.npz")


def _gold():
    """per case {min_length: arrays} in the layout of tests/golden/make_tracks_golden.py (no import of the library)"""
    g = dict(np.load(GOLD_PATH))
    at = {2: [0, 0], 3: [0, 0]}
    for c in range(len(g["case_n_pairs"])):
        want = {}
        for ml in (2, 3):
            n_t = int(g[f"n_tracks_{ml}"][c])
            t0, o0 = at[ml]
            length = g[f"track_len_{ml}"][t0:t0 + n_t].astype(np.int64)
            n_o = int(length.sum())
            want[ml] = dict(track_id=g[f"track_id_{ml}"][t0:t0 + n_t], track_len=length, obs_image=g[f"obs_image_{ml}"][o0:o0 + n_o],
                            obs_feature=g[f"obs_feature_{ml}"][o0:o0 + n_o])
            at[ml] = [t0 + n_t, o0 + n_o]
        yield want


def test_restatement_equals_the_compiled_reference():
    cases = tref.fixture_cases()
    gold = list(_gold())
    assert len(cases) == len(gold) == tref.N_FIXTURE
    for c, want in zip(cases, gold):
        for ml in (2, 3):
            own = tref.build(c["pairs"], c["match_start"], c["ij"], None, ml)
            assert np.array_equal(own.track_id, want[ml]["track_id"]), (c["name"], ml)
            assert np.array_equal(np.diff(own.track_start.astype(np.int64)), want[ml]["track_len"]), (c["name"], ml)
            assert np.array_equal(own.obs_image, want[ml]["obs_image"]) and np.array_equal(own.obs_feature, want[ml]["obs_feature"]), (c["name"], ml)


def test_fixture_inputs_are_the_generators():
    g = dict(np.load(GOLD_PATH))
    cases = tref.fixture_cases()
    assert np.array_equal(g["pairs"], np.concatenate([c["pairs"] for c in cases])) and np.array_equal(g["ij"], np.concatenate([c["ij"] for c in cases]))
    assert np.array_equal(g["match_start"], np.concatenate([c["match_start"] for c in cases]))
    assert np.array_equal(g["case_n_images"], [c["n_images"] for c in cases])
    assert np.array_equal(g["case_has_n_features"], [c["n_features"] is not None for c in cases])
    assert np.array_equal(g["n_features"], np.concatenate([c["n_features"] for c in cases if c["n_features"] is not None]))


def test_fixture_holds_what_the_device_tests_need():
    cases = tref.fixture_cases()
    collisions = short_at_3_only = other_root = 0
    for c in cases:
        two, three = (tref.build(c["pairs"], c["match_start"], c["ij"], None, ml) for ml in (2, 3))
        collisions += two.counts["n_collision"]
        short_at_3_only += three.counts["n_short"] - two.counts["n_short"]
        other_root += int((two.track_id != two.first_node).sum())
    assert collisions > 0 and short_at_3_only > 0
    assert other_root > 0   # the id of a track is the root of the reference's forest: a smallest-label implementation fails these
    assert any(c["n_features"] is not None for c in cases)
    assert any(c["n_features"] is None and c["ij"].size and int(c["ij"].max()) > 60000 for c in cases)   # sparse indices, n_features left out
    assert any(len(c["pairs"]) and c["n_images"] > int(c["pairs"].max()) + 1 for c in cases)            # an image without a match
    assert os.path.getsize(GOLD_PATH) <= 200 * 1024


def test_equal_rank_keeps_the_first_arguments_root():
    """union_find.hpp:91-102 by hand on three small containers; in the last the track's id is node 1, not its smallest node 0"""
    pairs, start, ij = tref.container({(0, 1): [(0, 0)], (1, 2): [(0, 0)]})
    got = tref.build(pairs, start, ij)
    assert np.array_equal(got.track_id, [0])   # container order: (0,1) first - node 0 is the first argument at equal rank
    pairs, start, ij = tref.container({(0, 2): [(0, 0)], (1, 2): [(0, 0)], (0, 1): []})
    got = tref.build(pairs, start, ij)   # (0,2): root 0 of {0, 2}, rank 1; (1,2): node 1 (rank 0) goes under 0
    assert np.array_equal(got.track_id, [0]) and np.array_equal(got.obs_image, [0, 1, 2])
    pairs, start, ij = tref.container({(1, 2): [(5, 5)], (0, 3): [(1, 1)], (2, 3): [(5, 1)]})
    got = tref.build(pairs, start, ij)   # nodes (0,1)=0 (1,5)=1 (2,5)=2 (3,1)=3; (0,3): root 0; (1,2): root 1; (2,3): Union(2, 3) -> roots 1, 0 at equal rank: 1 stays
    assert np.array_equal(got.track_id, [1]) and np.array_equal(got.first_node, [0])
