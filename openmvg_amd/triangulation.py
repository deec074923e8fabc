"""Triangulation of the tracks of a scene on the device (mvgx_triangulate_tracks).

  SfM_Data_Structure_Computation_Blind::triangulate          sfm/sfm_data_triangulation.cpp:166-222
  SfM_Data_Structure_Computation_Robust::robust_triangulation sfm/sfm_data_triangulation.cpp:319-434
  ETriangulationMethod                                        multiview/triangulation_method.hpp:15-22

The step between "tracks + poses" and the points bundle adjustment starts from. All numerics run in libmvgx_hip.so on the
GPU; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi

MODES = {"blind": _capi.MVGX_TRI_BLIND, "robust": _capi.MVGX_TRI_ROBUST}
# ETriangulationMethod; DEFAULT = INVERSE_DEPTH_WEIGHTED_MIDPOINT
METHODS = {"dlt": 0, "l1_angular": 1, "linfinity_angular": 2, "idw_midpoint": 3, "default": 3}


def default_options(**kw):
    o = _capi.TriangulateOptions()
    _capi.lib().mvgx_triangulate_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def triangulate_tracks(poses, intrinsics, intr_model, track_start, obs_pose, obs_intr, obs_xy, mode="robust", method="default",
                       max_reprojection_error=4.0, min_required_inliers=3, min_sample_index=3, obs_defined=None, device=-1):
    """Track t owns the observations [track_start[t], track_start[t + 1]), in the order of the reference's Observations map
    (ascending view id). poses (n, 6: angle-axis | t), intrinsics (m, 8) and intr_model (m) as in the BA scenes; obs_defined:
    0 for an observation whose view has no pose or intrinsic (None: all defined).
    Returns (X (n_tracks, 3; zeros for rejected tracks), track_ok (bool), obs_inlier (bool; blind: every observation of a kept
    track, robust: the inlier set), stats (_capi.TriangulateStats))."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 6)
    intrinsics = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, _capi.MVGX_BA_MAX_INTR_PARAMS)
    intr_model = np.ascontiguousarray(intr_model, np.int32).reshape(-1)
    if len(intr_model) != len(intrinsics):
        raise ValueError("intr_model and intrinsics differ in length")
    track_start = np.ascontiguousarray(track_start, np.uint64).reshape(-1)
    if len(track_start) < 1:
        raise ValueError("track_start needs n_tracks + 1 entries")
    n_tracks, n_obs = len(track_start) - 1, int(track_start[-1])
    obs_pose = np.ascontiguousarray(obs_pose, np.uint32).reshape(-1)
    obs_intr = np.ascontiguousarray(obs_intr, np.uint32).reshape(-1)
    obs_xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    if min(len(obs_pose), len(obs_intr), len(obs_xy)) < n_obs:
        raise ValueError("track_start runs past the observation arrays")
    if obs_defined is not None:
        obs_defined = np.ascontiguousarray(obs_defined, np.uint8).reshape(-1)
        if len(obs_defined) < n_obs:
            raise ValueError("track_start runs past obs_defined")
    opt = default_options(mode=MODES.get(mode, mode), method=METHODS.get(method, method), max_reprojection_error=float(max_reprojection_error),
                          min_required_inliers=int(min_required_inliers), min_sample_index=int(min_sample_index))
    X = np.zeros((n_tracks, 3))
    ok = np.zeros(n_tracks, np.uint8)
    inl = np.zeros(max(n_obs, len(obs_pose)), np.uint8)
    stats = _capi.TriangulateStats()
    _capi.check(_capi.lib().mvgx_triangulate_tracks(
        int(device), poses.ctypes.data, len(poses), intrinsics.ctypes.data, intr_model.ctypes.data, len(intrinsics), track_start.ctypes.data,
        n_tracks, obs_pose.ctypes.data, obs_intr.ctypes.data, obs_xy.ctypes.data, obs_defined.ctypes.data if obs_defined is not None else None,
        C.byref(opt), X.ctypes.data, ok.ctypes.data, inl.ctypes.data, C.byref(stats)))
    return X, ok.astype(bool), inl.astype(bool), stats


def scene_tracks(scene):
    """(order, track_start): the observations of a flat scene grouped by point - a stable sort, so the observations of a track keep
    the order they have in the scene (the reference's: ascending view id)."""
    obs_point = np.asarray(scene["obs_point"], np.int64)
    order = np.argsort(obs_point, kind="stable")
    counts = np.bincount(obs_point, minlength=int(scene["n_points"]))
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def triangulate_scene(scene, mode="robust", device=-1, **options):
    """SfM_Data_Structure_Computation_{Blind,Robust}::triangulate on the flat scene of openmvg_amd.ba / synth: the tracks (points
    and their observations) are triangulated from the scene's poses and intrinsics, rejected tracks are dropped with their
    observations, a robust run also drops the observations outside the inlier set, "points" receives the new positions and
    "obs_point" is renumbered. Returns (new scene, track_ok over the points of the input, stats); the new scene goes straight
    into ba.BaContext / Bundle_Adjustment_HIP.Adjust."""
    order, track_start = scene_tracks(scene)
    obs_xy = np.asarray(scene["obs_xy"], np.float64).reshape(-1, 2)
    X, ok, inl, stats = triangulate_tracks(scene["poses"], scene["intrinsics"], scene["intr_model"], track_start, np.asarray(scene["obs_pose"])[order],
                                           np.asarray(scene["obs_intr"])[order], obs_xy[order], mode=mode, device=device, **options)
    keep = order[inl[: len(order)]]
    new_id = np.cumsum(ok) - 1
    out = dict(scene)
    for k in ("obs_pose", "obs_intr", "obs_weight", "obs_is_control"):
        if scene.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(scene[k])[keep])
    out["obs_xy"] = np.ascontiguousarray(obs_xy[keep])
    out["obs_point"] = np.ascontiguousarray(new_id[np.asarray(scene["obs_point"], np.int64)[keep]].astype(np.uint32))
    out["points"] = np.ascontiguousarray(X[ok])
    if scene.get("point_const_mask") is not None:
        out["point_const_mask"] = np.ascontiguousarray(np.asarray(scene["point_const_mask"])[ok])
    out["n_points"] = int(ok.sum())
    out["n_obs"] = int(len(keep))
    return out, ok, stats
