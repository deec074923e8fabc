"""Relative pose of image pairs on the device (mvgx_relative_pose_from_essential, mvgx_relative_pose_robust).

  MotionFromEssential          multiview/essential.cpp:79-113
  RelativePoseFromEssential    multiview/motion_from_essential.cpp:20-95
  sfm::robustRelativePose      sfm/pipelines/sfm_robust_model_estimation.cpp:29-120
  Relative_Pose_Engine         sfm/pipelines/relative_pose_engine.cpp:87-223 (the tiny scene of :168-187: tiny_scene_points)

A batch of pairs per call; pair p owns the correspondences [start[p], start[p + 1]). All numerics run in libmvgx_hip.so on the GPU;
there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi
from .geofilter import pinhole_bearings
from .triangulation import METHODS

_RESULT = np.dtype([("pose", np.float64, (15,)), ("E", np.float64, (9,)), ("found_precision", np.float64), ("cheirality", np.uint32, (4,)),
                    ("n_acransac_inliers", np.uint32), ("n_selected", np.uint32), ("ok", np.uint32)], align=True)
assert _RESULT.itemsize == C.sizeof(_capi.RelativePoseResult)


class RelativePose_Info:
    """sfm::RelativePose_Info (sfm_robust_model_estimation.hpp) of one pair, and what RelativePoseFromEssential returns beside the pose:
    essential_matrix (3, 3), R (3, 3), t (3), center (3) - relativePose -, vec_inliers (the a-contrario inliers, ascending; None from
    from_essential), found_residual_precision, ok (the functions' return value; R, t, center are zeros where it is False), cheirality
    (points in front under each of the four candidate motions, in the library's candidate order: compare it sorted), selected (the
    positions the winner triangulated in front of both cameras) and points (their 3-D positions in the frame of the first camera)."""

    def __init__(self, row, selected, points, inliers=None):
        self.ok = bool(row["ok"])
        self.essential_matrix = row["E"].reshape(3, 3).copy()
        Rt = row["pose"][:12].reshape(3, 4)
        self.R, self.t, self.center = Rt[:, :3].copy(), Rt[:, 3].copy(), row["pose"][12:].copy()
        self.found_residual_precision = float(row["found_precision"])
        self.cheirality = tuple(int(v) for v in row["cheirality"])
        self.n_acransac_inliers = int(row["n_acransac_inliers"])
        self.vec_inliers = inliers
        self.selected, self.points = selected, points


def default_options(**kw):
    o = _capi.RelativePoseOptions()
    _capi.lib().mvgx_relative_pose_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _infos(res, sel_start, sel, X, masks=None):
    out = []
    for p in range(len(res)):
        lo, hi = int(sel_start[p]), int(sel_start[p + 1])
        out.append(RelativePose_Info(res[p], sel[lo:hi].copy(), X[lo:hi].copy(), None if masks is None else masks[p]))
    return out


def from_essential_raw(E, bI, bJ, start, use=None, method="default", ratio=0.7, device=-1):
    """mvgx_relative_pose_from_essential as it is -> (results structured array, selected_start, selected, X, stats).
    use: None (all correspondences of every pair in their order) or (use_start, use_index)."""
    E = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
    bI = np.ascontiguousarray(bI, np.float64).reshape(-1, 3)
    bJ = np.ascontiguousarray(bJ, np.float64).reshape(-1, 3)
    start = np.ascontiguousarray(start, np.uint64).reshape(-1)
    n_pairs = len(start) - 1
    if n_pairs < 0 or len(E) != n_pairs or len(bI) != len(bJ) or (n_pairs and int(start[-1]) > len(bI)):
        raise ValueError("from_essential: inconsistent array sizes")
    use_start = use_index = None
    n_list = int(start[-1]) if n_pairs else 0
    if use is not None:
        use_start = np.ascontiguousarray(use[0], np.uint64).reshape(-1)
        use_index = np.ascontiguousarray(use[1], np.uint32).reshape(-1)
        if len(use_start) != n_pairs + 1 or int(use_start[-1]) > len(use_index):
            raise ValueError("from_essential: use_start does not fit the pairs or the index list")
        if len(use_index) == 0:
            use_index = np.zeros(1, np.uint32)   # (an empty list is still a list: a pointer, not NULL)
        n_list = int(use_start[-1])
    opt = default_options(method=METHODS.get(method, method), positive_depth_ratio=float(ratio))
    res = np.zeros(max(n_pairs, 1), _RESULT)
    sel_start = np.zeros(n_pairs + 1, np.uint64)
    sel = np.zeros(max(n_list, 1), np.uint32)
    X = np.zeros((max(n_list, 1), 3))
    stats = _capi.RelativePoseStats()
    _capi.check(_capi.lib().mvgx_relative_pose_from_essential(int(device), n_pairs, _ptr(start), _ptr(bI), _ptr(bJ), _ptr(E), _ptr(use_start), _ptr(use_index),
                                                              C.byref(opt), _ptr(res), _ptr(sel_start), _ptr(sel), _ptr(X), C.byref(stats)))
    return res[:n_pairs], sel_start, sel, X, stats


def from_essential(E, bI, bJ, start, use=None, method="default", ratio=0.7, device=-1):
    """RelativePoseFromEssential for every pair: E (n_pairs, 3, 3), bearing vectors bI / bJ (N, 3), pair p owning rows [start[p],
    start[p + 1]). use: None - vote with all correspondences - or one index array per pair (positions within the pair, any order, a
    subset: bearing_vector_index_to_use). Returns a list of RelativePose_Info."""
    if use is not None:
        lists = [np.asarray(u, np.uint32).reshape(-1) for u in use]
        use = (np.concatenate([[0], np.cumsum([len(u) for u in lists])]).astype(np.uint64),
               np.concatenate(lists) if lists else np.zeros(0, np.uint32))
    res, sel_start, sel, X, _ = from_essential_raw(E, bI, bJ, start, use, method, ratio, device)
    return _infos(res, sel_start, sel, X)


def _robust(kind, head, n_matches, n_pairs, tolerance, max_iterations, method, ratio, device, start):
    opt = default_options(kind=kind, method=METHODS.get(method, method), positive_depth_ratio=float(ratio), residual_tolerance=float(tolerance),
                          max_iterations=int(max_iterations))
    mask = np.zeros(max(n_matches, 1), np.uint8)
    res = np.zeros(max(n_pairs, 1), _RESULT)
    sel_start = np.zeros(n_pairs + 1, np.uint64)
    sel = np.zeros(max(n_matches, 1), np.uint32)
    X = np.zeros((max(n_matches, 1), 3))
    stats = _capi.RelativePoseStats()
    _capi.check(_capi.lib().mvgx_relative_pose_robust(int(device), *map(_ptr, head), n_pairs, C.byref(opt), _ptr(mask), _ptr(res), _ptr(sel_start), _ptr(sel),
                                                      _ptr(X), C.byref(stats)))
    mask = mask[:n_matches].astype(bool)
    inl = [np.flatnonzero(mask[int(start[p]):int(start[p + 1])]).astype(np.uint32) for p in range(n_pairs)]
    return _infos(res[:n_pairs], sel_start, sel, X, inl), mask, stats


def robust(xI, xJ, start, image_wh, K, tolerance=2.5 * 2.5, max_iterations=256, method="default", ratio=0.7, bearings=None, device=-1):
    """robustRelativePose for pairs of pinhole cameras: pixels xI / xJ (N, 2) with the distortion removed, image_wh (n_pairs, 4) {w_I, h_I,
    w_J, h_J}, K (n_pairs, 2, 3, 3); tolerance = RelativePose_Info::initial_residual_tolerance, SQUARED pixels (Square(2.5) with 256
    iterations in the global engine, Square(4.0) with 4096 in the sequential one); bearings = (bI, bJ) or None: pinhole_bearings.
    Returns (list of RelativePose_Info, the a-contrario inlier mask (N,), stats)."""
    xI = np.ascontiguousarray(xI, np.float64).reshape(-1, 2)
    xJ = np.ascontiguousarray(xJ, np.float64).reshape(-1, 2)
    start = np.ascontiguousarray(start, np.uint64).reshape(-1)
    n_pairs = len(start) - 1
    wh = np.ascontiguousarray(image_wh, np.uint32).reshape(-1, 4)
    K = np.ascontiguousarray(K, np.float64).reshape(-1, 18)
    if n_pairs < 0 or len(wh) != n_pairs or len(K) != n_pairs or int(start[-1]) != len(xI) or len(xI) != len(xJ):
        raise ValueError("robust: inconsistent array sizes")
    if bearings is None:
        bI = np.zeros((len(xI), 3)); bJ = np.zeros((len(xJ), 3))
        for p in range(n_pairs):
            lo, hi = int(start[p]), int(start[p + 1])
            bI[lo:hi] = pinhole_bearings(K[p, :9], xI[lo:hi]); bJ[lo:hi] = pinhole_bearings(K[p, 9:], xJ[lo:hi])
    else:
        bI, bJ = (np.ascontiguousarray(b, np.float64).reshape(-1, 3) for b in bearings)
    return _robust(_capi.MVGX_RELPOSE_PINHOLE, [xI, xJ, bI, bJ, start, wh, K], len(xI), n_pairs, tolerance, max_iterations, method, ratio, device, start)


def robust_angular(bI, bJ, start, tolerance_deg=4.0, max_iterations=256, method="default", ratio=0.7, device=-1):
    """robustRelativePose for cameras that are not pinholes (spherical): the eight-point solver with the angular error on the bearing
    vectors alone; tolerance_deg = initial_residual_tolerance in degrees. Returns as robust(); found_residual_precision in degrees."""
    bI = np.ascontiguousarray(bI, np.float64).reshape(-1, 3)
    bJ = np.ascontiguousarray(bJ, np.float64).reshape(-1, 3)
    start = np.ascontiguousarray(start, np.uint64).reshape(-1)
    n_pairs = len(start) - 1
    if n_pairs < 0 or int(start[-1]) != len(bI) or len(bI) != len(bJ):
        raise ValueError("robust_angular: inconsistent array sizes")
    return _robust(_capi.MVGX_RELPOSE_ANGULAR, [None, None, bI, bJ, start, None, None], len(bI), n_pairs, tolerance_deg, max_iterations, method, ratio, device, start)


def essential_from_pose(R, t):
    """[t]x R of a relative pose (multiview/essential.cpp:66-76 with the first camera at the origin)"""
    t = np.asarray(t, np.float64).reshape(3)
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]) @ np.asarray(R, np.float64).reshape(3, 3)


def tiny_scene_points(infos, bI, bJ, start, method="default", ratio=0.7, device=-1):
    """The structure Relative_Pose_Engine::Process gives the two-view scene of every pair (relative_pose_engine.cpp:168-187): ALL matches
    of the pair triangulated under the pose that won - a second from_essential call with use = None and the winning pose's E. Pairs that
    are not ok vote with a zero matrix and come back not ok. Returns a list of RelativePose_Info (selected = the landmarks' match
    positions, points = their X)."""
    E = np.stack([essential_from_pose(i.R, i.t) if i.ok else np.zeros((3, 3)) for i in infos]) if infos else np.zeros((0, 3, 3))
    return from_essential(E, bI, bJ, start, None, method, ratio, device)
