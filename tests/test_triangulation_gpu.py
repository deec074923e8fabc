"""GPU: mvgx_triangulate_tracks on the MI355X against the float64 restatement of the reference (tests/_triangulation_ref.py): decisions
equal, points within the tolerance of tests/_triangulation_cases.py. The CPU twin (emulation) is tests/test_triangulation_emu_cpu.py."""
import math

import numpy as np
import pytest

from openmvg_amd import ba, synth, triangulation
from tests import _triangulation_cases as cases
from tests import _triangulation_ref as ref

pytestmark = pytest.mark.gpu


# Seeds of the six scenes below. With 2 000 tracks the smallest gap between a hypothesis error and the best error it is compared with is
# a few 1e-6 on a typical draw; 703 and 705 gave 4.1e-7 and 5.5e-7, below the guard on the inputs (cases.MIN_MARGIN), and were replaced.
SHORT_SCENE_SEED = {ref.PINHOLE: 701, ref.RADIAL1: 702, ref.RADIAL3: 803, ref.BROWN: 704, ref.FISHEYE: 805, ref.SPHERICAL: 707}


def _short_scene(model):
    """8 poses, 2 000 tracks of 2 .. 12 observations (tracks longer than 8 see some poses from two views)"""
    return ref.scene(8, cases.mixed_lengths(2000, 2, 12, seed=31), model=model, seed=SHORT_SCENE_SEED[model])


@pytest.mark.parametrize("model", ref.MODELS)
def test_blind_short_tracks(built_lib, model):
    (_, ok, _, _), _, _ = cases.compare(f"gpu-short-{model}", _short_scene(model), mode="blind")
    assert ok.sum() >= 1900


@pytest.mark.parametrize("model", ref.MODELS)
def test_robust_short_tracks(built_lib, model):
    sc = _short_scene(model)
    (_, ok, inl, stats), _, _ = cases.compare(f"gpu-short-{model}", sc)
    n = np.diff(sc["track_start"].astype(np.int64))
    assert ok[n >= 3].mean() > 0.95 and not ok[n == 2].any()   # (3, 3): two views are too few, nearly every other track of the family is kept
    assert not inl[sc["displaced"]].any()
    assert stats.n_hypotheses == 2 * n[n > 3].sum()    # the tracks that reach the loop (n == 3 is the all-observations case)


@pytest.mark.parametrize("need,k", [(2, 2), (3, 2)])
def test_robust_two_view_samples(built_lib, need, k):
    sc = ref.scene(12, cases.mixed_lengths(400, 2, 12, seed=37), seed=800 + need)
    for method in (ref.DLT, ref.L1_ANGULAR, ref.LINF_ANGULAR, ref.IDW_MIDPOINT):
        (_, ok, _, _), _, _ = cases.compare(f"gpu-two-view-{need}", sc, method=method, min_required_inliers=need, min_sample_index=k)
        assert ok.sum() >= 300


@pytest.mark.parametrize("mode", ["blind", "robust"])
def test_long_tracks(built_lib, mode):
    """72 cameras, 64 tracks of 33 .. 70 observations: rounds of 64 hypotheses, and above 64 observations records from global memory"""
    sc = ref.scene(72, cases.mixed_lengths(64, 33, 70, seed=41), seed=900)
    (_, ok, _, stats), _, _ = cases.compare("gpu-long", sc, mode=mode)
    assert ok.all()
    if mode == "robust":
        assert stats.n_hypotheses == 2 * np.diff(sc["track_start"].astype(np.int64)).sum()


def test_repeatable_and_order_independent(built_lib):
    sc = ref.scene(72, cases.mixed_lengths(500, 2, 70, seed=43), seed=1000)
    X, ok, inl, _ = cases.run_device(sc)
    X2, ok2, inl2, _ = cases.run_device(sc)
    assert np.array_equal(X, X2) and np.array_equal(ok, ok2) and np.array_equal(inl, inl2)
    perm = np.random.default_rng(0).permutation(500)
    n = np.diff(sc["track_start"].astype(np.int64))
    order = np.concatenate([np.arange(int(sc["track_start"][t]), int(sc["track_start"][t + 1])) for t in perm])
    sp = dict(sc, track_start=np.concatenate([[0], np.cumsum(n[perm])]).astype(np.uint64), obs_pose=sc["obs_pose"][order],
              obs_intr=sc["obs_intr"][order], obs_xy=sc["obs_xy"][order])
    Xp, okp, inlp, _ = cases.run_device(sp)
    assert np.array_equal(Xp, X[perm]) and np.array_equal(okp, ok[perm]) and np.array_equal(inlp, inl[order])
    assert ok.sum() >= 400


# ---- form edges: the bodies are in tests/_triangulation_cases.py and run under the emulation too. What only real waves decide: shuffles
# across lanes that left the hypothesis loop early, the one barrier after the LDS staging, the 64-bit inlier mask, the lanes of a 16-lane
# group without a track. A view without pose names an extra pose row and an extra intrinsic row of NaNs here - every index the device
# can read is in range, and an unguarded read shows as a wrong decision. ----
@pytest.mark.parametrize("need,k", cases.ROBUST_FORMS)
def test_robust_group_boundaries(built_lib, need, k):
    cases.check_group_boundaries(need, k, poison=True)


@pytest.mark.parametrize("model", ref.MODELS)
def test_blind_rejections(built_lib, model):
    cases.check_blind_rejections(model, poison=True)


@pytest.mark.parametrize("model", ref.MODELS)
def test_robust_behind_the_camera(built_lib, model):
    cases.check_robust_behind(model)


def test_views_without_pose(built_lib):
    cases.check_views_without_pose(poison=True)


def test_mixed_cameras(built_lib):
    cases.check_mixed_cameras()


def test_ragged_groups(built_lib):
    cases.check_ragged_groups()


@pytest.mark.parametrize("need,k", cases.OTHER_FORMS)
def test_other_caller_forms(built_lib, need, k):
    cases.check_other_caller_form(need, k)


def test_offset_observation_arrays(built_lib):
    cases.check_offset_observation_arrays()


def test_degenerate_two_view_input(built_lib):
    cases.check_degenerate_pairs()


@pytest.mark.parametrize("need,k", [(2, 2), (3, 2)])
def test_two_view_samples_sharing_a_pose(built_lib, need, k):
    cases.check_samples_sharing_a_pose(need, k)


def test_output_feeds_bundle_adjustment(built_lib):
    """tracks + true poses -> triangulate_scene -> ba.BaContext: the solve starts from a finite cost near the noise level"""
    scene = synth.ba_scene(16, 400, track_len=5, seed=5)
    scene = dict(scene, poses=scene["poses_gt"], intrinsics=scene["intrinsics_gt"], points=np.zeros_like(scene["points"]))
    out, ok, stats = triangulation.triangulate_scene(scene)
    assert ok.sum() >= 380 and out["n_points"] == int(ok.sum()) and out["n_obs"] == stats.n_inlier_obs
    assert np.abs(out["points"] - scene["points_gt"][ok]).max() < 0.05
    ctx = ba.BaContext(out)
    try:
        summary = ctx.solve(ba.default_options(max_num_iterations=3))
    finally:
        ctx.close()
    assert math.isfinite(summary.initial_cost) and summary.initial_rmse < 2.0   # pixel noise 0.5 per axis
    assert summary.final_cost <= summary.initial_cost
