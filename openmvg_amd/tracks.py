"""Feature tracks from pairwise matches on the device (mvgx_tracks_build).

  tracks::TracksBuilder::Build / Filter / ExportToSTL   tracks/tracks.hpp:62-197
  UnionFind::Union                                       tracks/union_find.hpp:75-103

The step between the matchers + the geometric filter and triangulation: `build` fuses the pairwise match lists into tracks with the
reference's track ids, `observations` turns them into the arrays `triangulation.triangulate_tracks` takes. All of `build` runs in
libmvgx_hip.so on the GPU; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi


class Tracks:
    """track_id (n_tracks, ascending: the node index of each track's root in the reference's forest), track_start (n_tracks + 1
    offsets), obs_image / obs_feature (one entry per observation, ascending image inside a track), stats (_capi.TracksStats)."""

    def __init__(self, track_id, track_start, obs_image, obs_feature, stats):
        self.track_id, self.track_start, self.obs_image, self.obs_feature, self.stats = track_id, track_start, obs_image, obs_feature, stats

    def __len__(self):
        return len(self.track_id)


def _take(pointer, count, dtype):
    """copies `count` values out of an array the library allocated, then releases it"""
    try:
        if not count:
            return np.zeros(0, dtype)
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,)).copy()
    finally:
        _capi.lib().mvgx_host_free(pointer)


def build(pairs, match_start, ij, n_images=None, n_features=None, match_mask=None, min_length=2, device=-1):
    """pairs (n_pairs, 2: I < J, ascending), match_start (n_pairs + 1), ij (n_matches, 2) - what the matchers return and the indexed
    filter entries take; match_mask: a uint8 per match, 0 drops it (a filter's inlier_mask as it is). n_images: None = the largest
    image index used + 1 (or len(n_features)); n_features: per image, None = from the indices used. Returns a Tracks."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    match_start = np.ascontiguousarray(match_start, np.uint64).reshape(-1)
    ij = np.ascontiguousarray(ij, np.uint32).reshape(-1, 2)
    n_pairs = len(pairs)
    if len(match_start) != n_pairs + 1 and (n_pairs or len(match_start)):
        raise ValueError("match_start needs n_pairs + 1 entries")
    if n_pairs and int(match_start.max()) > len(ij):
        raise ValueError("match_start runs past ij")
    if match_mask is not None:
        match_mask = np.ascontiguousarray(match_mask, np.uint8).reshape(-1)
        if len(match_mask) < len(ij):
            raise ValueError("match_mask is shorter than ij")
    if n_features is not None:
        n_features = np.ascontiguousarray(n_features, np.uint32).reshape(-1)
    if n_images is None:
        n_images = len(n_features) if n_features is not None else (int(pairs.max()) + 1 if n_pairs else 0)
    if n_features is not None and len(n_features) != n_images:
        raise ValueError("n_features needs one entry per image")
    opt = _capi.TracksOptions()
    lib = _capi.lib()
    lib.mvgx_tracks_default_options(C.byref(opt))
    opt.min_length = int(min_length)
    n_tracks = C.c_uint32(0)
    p_id, p_start, p_image, p_feature = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    stats = _capi.TracksStats()
    _capi.check(lib.mvgx_tracks_build(int(device), int(n_images), n_features.ctypes.data if n_features is not None else None,
                                      pairs.ctypes.data if n_pairs else None, match_start.ctypes.data if n_pairs else None, ij.ctypes.data if len(ij) else None,
                                      match_mask.ctypes.data if match_mask is not None and len(match_mask) else None, n_pairs, C.byref(opt), C.byref(n_tracks),
                                      C.byref(p_id), C.byref(p_start), C.byref(p_image), C.byref(p_feature), C.byref(stats)))
    n = n_tracks.value
    track_start = _take(p_start, n + 1, np.uint64)
    n_obs = int(track_start[-1])
    return Tracks(_take(p_id, n, np.uint32), track_start, _take(p_image, n_obs, np.uint32), _take(p_feature, n_obs, np.uint32), stats)


def observations(tracks, feat_xy, feat_start, view_pose, view_intr):
    """The observation arrays of `tracks` in the order triangulation.triangulate_tracks expects (track after track, ascending view):
    feat_xy (all features of all images, 2 doubles each) and feat_start (n_images + 1 offsets into it) as the indexed filter entries
    take them; view_pose / view_intr: per image the index of its pose / intrinsic, negative = none yet.
    Returns (obs_pose, obs_intr, obs_xy, obs_defined); a view without pose or intrinsic comes out with obs_defined = 0 (and index 0).
    A host-side gather: matches -> build -> observations -> triangulate_tracks needs no code in between."""
    feat_xy = np.asarray(feat_xy, np.float64).reshape(-1, 2)
    feat_start = np.asarray(feat_start, np.int64).reshape(-1)
    view_pose = np.asarray(view_pose, np.int64).reshape(-1)
    view_intr = np.asarray(view_intr, np.int64).reshape(-1)
    image = tracks.obs_image.astype(np.int64)
    feature = tracks.obs_feature.astype(np.int64)
    if len(image) and (int(image.max()) >= min(len(view_pose), len(view_intr), len(feat_start) - 1) or np.any(feature >= feat_start[image + 1] - feat_start[image])):
        raise ValueError("the tracks name an image or a feature the arrays do not hold")
    pose, intr = view_pose[image], view_intr[image]
    defined = (pose >= 0) & (intr >= 0)
    obs_xy = np.ascontiguousarray(feat_xy[feat_start[image] + feature]).reshape(-1, 2)
    return (np.where(defined, pose, 0).astype(np.uint32), np.where(defined, intr, 0).astype(np.uint32), obs_xy, defined.astype(np.uint8))
