"""CPU, no library: the float64 restatement of MotionFromEssential + RelativePoseFromEssential (tests/_relative_pose_ref.py) against the
compiled reference's outputs in tests/golden/relative_pose_golden.npz, and the construction of the ratio edge on the restatement alone."""
import os

import numpy as np
import pytest

from tests import _relative_pose_ref as rref

GOLD = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relative_pose_golden.npz")))


def _cases():
    first = np.concatenate([[0], np.cumsum(GOLD["stage_n"])])
    at_use = at_sel = 0
    for i in range(len(GOLD["stage_key"])):
        rec, un, k = int(GOLD["stage_input"][i]), int(GOLD["stage_use_n"][i]), int(GOLD["stage_n_selected"][i])
        lo, hi = int(first[rec]), int(first[rec + 1])
        yield dict(key=tuple(int(v) for v in GOLD["stage_key"][i]), method=int(GOLD["stage_method"][i]), ratio=float(GOLD["stage_ratio"][i]), E=GOLD["stage_E"][rec],
                   bI=GOLD["stage_bI"][lo:hi], bJ=GOLD["stage_bJ"][lo:hi], use=None if un < 0 else GOLD["stage_use"][at_use:at_use + un], ok=bool(GOLD["stage_ok"][i]),
                   counts=tuple(int(v) for v in GOLD["stage_counts"][i]), pose=GOLD["stage_pose"][i], selected=GOLD["stage_selected"][at_sel:at_sel + k],
                   points=GOLD["stage_points"][at_sel:at_sel + k])
        at_use += max(un, 0); at_sel += k


def test_restatement_against_the_compiled_reference():
    """decisions equal above the guard, at most 5 % of the cases below it, pose and points inside the spread the generator recorded"""
    spread_pose, spread_points = (float(v) for v in GOLD["spread"])
    below = n = 0
    for c in _cases():
        n += 1
        own = rref.relative_pose_from_essential(c["bI"], c["bJ"], c["E"], c["use"], c["ratio"], c["method"])
        if own.point_margin < float(GOLD["guard"]):
            below += 1
            continue
        assert own.ok == c["ok"] and sorted(own.cheirality) == sorted(c["counts"]), c["key"]
        if own.ok:
            assert np.array_equal(own.selected, c["selected"]), c["key"]
            assert np.abs(np.concatenate([own.R.ravel(), own.t, own.center]) - c["pose"]).max() <= spread_pose, c["key"]
            if len(own.points):
                assert (np.abs(own.points - c["points"]).max(axis=1) / np.maximum(1.0, np.abs(c["points"]).max(axis=1))).max() <= spread_points, c["key"]
    assert n == 64 and below <= 0.05 * n


def test_fixture_holds_the_constructions():
    """the reference's own counts on the ratio edge and on the pair without a solution"""
    for c in _cases():
        if c["key"][0] == 1:
            m, k = c["key"][2], c["key"][3]
            assert sorted(c["counts"]) == sorted((m, k, 0, 0)) and c["ok"] == ((m, k) in ((10, 6), (17, 3))), c["key"]
        if c["key"][0] == 2:
            assert not c["ok"] and max(c["counts"]) == 0   # (the pose beside it is the driver's default Pose3: the reference exports none)


@pytest.mark.parametrize("method", range(4))
def test_ratio_edge_construction(method):
    from tests._relative_pose_ref import RATIO_CASES, essential, ratio_pair, relative_pose_from_essential
    rng = np.random.default_rng([rref.SEED, 50 + method])
    for m, k in RATIO_CASES:
        R, t, bI, bJ, majority = ratio_pair(m, k, rng)
        E = essential(R, t)
        assert float(np.abs(np.einsum("ni,ij,nj->n", bJ, E, bI)).max()) < 1e-15   # residuals of 1e-16
        own = relative_pose_from_essential(bI, bJ, E, None, 0.7, method)
        assert sorted(own.cheirality) == sorted((m, k, 0, 0)), (m, k, own.cheirality)
        assert own.ok == ((m, k) in ((10, 6), (17, 3))), (m, k)   # 7 / 10.0 < 0.7 and 14 / 20.0 < 0.7 are false in double
        if own.ok:
            assert np.array_equal(own.selected, majority) and np.abs(own.R - R).max() < 1e-12 and np.abs(own.t - t).max() < 1e-12


def test_robust_fixture_shape():
    n_pairs = len(GOLD["robust_start"]) - 1
    assert n_pairs == 25 and GOLD["robust_ok"].shape == (2, n_pairs)
    assert int(GOLD["robust_n_inliers"].sum()) == len(GOLD["robust_inliers"])
    assert not GOLD["robust_ok"][:, -1].any() and (GOLD["robust_n_inliers"][:, -1] < 13).all()   # the pair of 12 good correspondences
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relative_pose_golden.npz")) <= \
        os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resection_dlt_golden.npz"))
