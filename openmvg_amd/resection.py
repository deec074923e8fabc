"""Robust camera resection on the device (mvgx_resection_localize, mvgx_resection_localize_bounded, mvgx_resection_localize_uncalibrated):
a batch of independent problems.

  SfM_Localizer::Localize (error_max = infinity)   sfm/pipelines/localization/SfM_Localizer.cpp:109-343      localize
  SfM_Localizer::Localize (a finite error_max)      the same, ACRANSAC in its quantified form                 localize_bounded
  ACRANSAC, exhaustive NFA                          robust_estimation/robust_estimator_ACRansac.hpp:257-304, :326-489
  ACRANSAC, quantified NFA, warm-up, early exit     robust_estimation/robust_estimator_ACRansac.hpp:205-256, :351-358, :375-475
  P3PSolver_Ding / P3PSolver_Nordberg               multiview/solver_resection_p3p_{ding,nordberg}.cpp
  KRt_From_P                                        multiview/projection.cpp:40-132
  SfM_Localizer::Localize, a view without intrinsics sfm/pipelines/localization/SfM_Localizer.cpp:134-161, :321-331   localize_uncalibrated
  ACKernelAdaptorResection, UnnormalizerResection   robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:203-288
  NormalizePoints by the image size                 multiview/conditioning.cpp:54-77
  SixPointResectionSolver                           multiview/solver_resection_kernel.cpp:29-136                     dlt6
  the intrinsics the engine creates from P          sfm/pipelines/sequential/sequential_SfM.cpp:979-1021             intrinsic_seed

The step that starts every round of the sequential pipeline: a view is resected against the points reconstructed so far. All numerics run
in libmvgx_hip.so on the GPU; there is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np

from . import _capi

# resection::SolverType (multiview/solver_resection.hpp:15-24); the two P3P solvers have a device path in localize / localize_bounded,
# dlt6 in localize_uncalibrated
SOLVERS = {"dlt6": 0, "ke": 1, "kneip": 2, "nordberg": 3, "ding": 4, "up2p": 5, "default": 4}


def default_options(**kw):
    o = _capi.ResectionOptions()
    _capi.lib().mvgx_resection_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Localization:
    """The result of one problem. ok: more than 2.5 * 3 inliers; R, t, C: KRt_From_P of the winning model and the centre (ok only);
    P: the solver's [R | t] (3 x 4, ok only); error_max: the a-contrario threshold in pixels; inliers: indices in ascending residual (localize) or ascending index (localize_bounded)."""

    def __init__(self, ok, pose, P, error_max, min_nfa, inliers, K=None):
        self.ok = bool(ok)
        self.R = pose[:12].reshape(3, 4)[:, :3].copy() if ok else None
        self.t = pose[:12].reshape(3, 4)[:, 3].copy() if ok else None
        self.C = pose[12:15].copy() if ok else None
        self.P = P.reshape(3, 4).copy() if ok else None
        self.error_max = float(error_max)
        self.min_nfa = float(min_nfa)
        self.inliers = inliers
        if K is not None:   # localize_uncalibrated: P is the unnormalised projection matrix, K the calibration of KRt_From_P(P)
            self.K = K.reshape(3, 3).copy() if ok else None


TRACE_RECORD = 10   # words of a trace record: iteration | k | the first 8 indices of the sorted list


def _call(entry, device, start, x2d, X3d, intr_model, intrinsics, opt, trace_events=0):
    """the arrays of one call of either entry; returns (list of Localization, stats)"""
    start = np.ascontiguousarray(start, np.uint64).reshape(-1)
    if len(start) < 1:
        raise ValueError("start needs n_problems + 1 entries")
    n_problems = len(start) - 1
    x2d = np.ascontiguousarray(x2d, np.float64).reshape(-1, 2)
    X3d = np.ascontiguousarray(X3d, np.float64).reshape(-1, 3)
    if n_problems and min(len(x2d), len(X3d)) < int(start.max()):
        raise ValueError("start runs past the correspondence arrays")
    intr_model = np.ascontiguousarray(intr_model, np.int32).reshape(-1)
    intrinsics = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, _capi.MVGX_BA_MAX_INTR_PARAMS)
    if len(intr_model) != n_problems or len(intrinsics) != n_problems:
        raise ValueError("one camera model and one intrinsics row per problem")
    ok = np.zeros(n_problems, np.uint8)
    pose = np.zeros((n_problems, 15))
    P = np.zeros((n_problems, 12))
    err = np.zeros(n_problems)
    nfa = np.zeros(n_problems)
    inl_start = np.zeros(n_problems + 1, np.uint64)
    inl = np.zeros(max(len(x2d), 1), np.uint32)
    stats = _capi.ResectionStats()
    trace = None
    if trace_events:
        trace = np.zeros((n_problems, 1 + TRACE_RECORD * int(trace_events)), np.uint32)
        fn = _capi.lib().mvgx_resection_debug_trace
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32]
        _capi.check(fn(trace.ctypes.data, int(trace_events)))
    _capi.check(getattr(_capi.lib(), entry)(
        int(device), n_problems, start.ctypes.data, x2d.ctypes.data, X3d.ctypes.data, intr_model.ctypes.data, intrinsics.ctypes.data, C.byref(opt),
        ok.ctypes.data, pose.ctypes.data, P.ctypes.data, err.ctypes.data, nfa.ctypes.data, inl_start.ctypes.data, inl.ctypes.data, C.byref(stats)))
    out = [Localization(ok[p], pose[p], P[p], err[p], nfa[p], inl[int(inl_start[p]):int(inl_start[p + 1])].copy()) for p in range(n_problems)]
    if trace is not None:
        for p, loc in enumerate(out):
            recs = trace[p, 1:].reshape(-1, TRACE_RECORD)[: min(int(trace[p, 0]), int(trace_events))]
            loc.better = [(int(r[0]), int(r[1]), [int(v) for v in r[2:2 + min(int(r[1]), TRACE_RECORD - 2)]]) for r in recs]
            loc.better_count = int(trace[p, 0])
    return out, stats


def _options(solver, max_iteration, error_max, waves_ahead, global_above):
    return default_options(solver=SOLVERS.get(solver, solver), max_iteration=int(max_iteration), error_max=float(error_max),
                          waves_ahead=int(waves_ahead), global_above=int(global_above))


def localize(start, x2d, X3d, intr_model, intrinsics, solver="ding", max_iteration=4096, error_max=math.inf, device=-1, waves_ahead=0,
             global_above=0, trace_events=0):
    """Problem p owns the correspondences [start[p], start[p + 1]) of x2d (pixels, distortion already removed) and X3d; intr_model[p] and
    intrinsics[p] (8 values, the BA scenes' layout) are its camera. Returns (list of Localization, _capi.ResectionStats).
    error_max must be infinity here (the exhaustive NFA); a finite bound is localize_bounded's.
    waves_ahead / global_above: test hooks that select the kernel's form; they do not change any result. trace_events > 0 (test hook
    mvgx_resection_debug_trace): every Localization also gets .better = [(iteration, k, head of the sorted list)] for the first
    trace_events iterations that found a better model."""
    return _call("mvgx_resection_localize", device, start, x2d, X3d, intr_model, intrinsics,
                 _options(solver, max_iteration, error_max, waves_ahead, global_above), trace_events)


def localize_bounded(start, x2d, X3d, intr_model, intrinsics, error_max, solver="ding", max_iteration=4096, device=-1, waves_ahead=0, global_above=0):
    """SfM_Localizer::Localize with a finite error_max (mvgx_resection_localize_bounded): the bound in pixels, finite and > 0. AC-RANSAC
    reads the NFA off a 20-bin histogram below the bound, warms up as a max-consensus loop and gives up early when no model has more than
    2.5 * 3 residuals inside the bound. Arguments and return value as localize's; Localization.error_max is the threshold found (one of
    19 steps of the bound) and Localization.inliers are in ascending index order."""
    return _call("mvgx_resection_localize_bounded", device, start, x2d, X3d, intr_model, intrinsics,
                 _options(solver, max_iteration, error_max, waves_ahead, global_above))


def localize_uncalibrated(start, x2d, X3d, image_wh, max_iteration=4096, device=-1, waves_ahead=0, global_above=0, trace_events=0):
    """SfM_Localizer::Localize for views WITHOUT intrinsics (mvgx_resection_localize_uncalibrated): AC-RANSAC over the six-point DLT solver.
    Problem p owns the correspondences [start[p], start[p + 1]) of x2d (the pixels as measured) and X3d; image_wh[p] = (width, height) of
    its view. Returns (list of Localization, _capi.ResectionStats); a Localization here has ok = more than 2.5 * 6 inliers, P = the
    unnormalised 3 x 4 projection matrix, K, R, t, C = KRt_From_P(P) (K / K(2,2)), error_max in pixels, inliers in ascending residual.
    waves_ahead / global_above / trace_events: the test hooks of localize."""
    start = np.ascontiguousarray(start, np.uint64).reshape(-1)
    if len(start) < 1:
        raise ValueError("start needs n_problems + 1 entries")
    n_problems = len(start) - 1
    x2d = np.ascontiguousarray(x2d, np.float64).reshape(-1, 2)
    X3d = np.ascontiguousarray(X3d, np.float64).reshape(-1, 3)
    if n_problems and min(len(x2d), len(X3d)) < int(start.max()):
        raise ValueError("start runs past the correspondence arrays")
    image_wh = np.ascontiguousarray(image_wh, np.uint32).reshape(-1, 2)
    if len(image_wh) != n_problems:
        raise ValueError("one (width, height) per problem")
    opt = _options("dlt6", max_iteration, math.inf, waves_ahead, global_above)
    ok = np.zeros(n_problems, np.uint8)
    pose = np.zeros((n_problems, 15))
    P = np.zeros((n_problems, 12))
    K = np.zeros((n_problems, 9))
    err = np.zeros(n_problems)
    nfa = np.zeros(n_problems)
    inl_start = np.zeros(n_problems + 1, np.uint64)
    inl = np.zeros(max(len(x2d), 1), np.uint32)
    stats = _capi.ResectionStats()
    trace = None
    if trace_events:
        trace = np.zeros((n_problems, 1 + TRACE_RECORD * int(trace_events)), np.uint32)
        fn = _capi.lib().mvgx_resection_debug_trace
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32]
        _capi.check(fn(trace.ctypes.data, int(trace_events)))
    _capi.check(_capi.lib().mvgx_resection_localize_uncalibrated(
        int(device), n_problems, start.ctypes.data, x2d.ctypes.data, X3d.ctypes.data, image_wh.ctypes.data, C.byref(opt), ok.ctypes.data,
        pose.ctypes.data, P.ctypes.data, K.ctypes.data, err.ctypes.data, nfa.ctypes.data, inl_start.ctypes.data, inl.ctypes.data, C.byref(stats)))
    out = [Localization(ok[p], pose[p], P[p], err[p], nfa[p], inl[int(inl_start[p]):int(inl_start[p + 1])].copy(), K=K[p]) for p in range(n_problems)]
    if trace is not None:
        for p, loc in enumerate(out):
            recs = trace[p, 1:].reshape(-1, TRACE_RECORD)[: min(int(trace[p, 0]), int(trace_events))]
            loc.better = [(int(r[0]), int(r[1]), [int(v) for v in r[2:2 + min(int(r[1]), TRACE_RECORD - 2)]]) for r in recs]
            loc.better_count = int(trace[p, 0])
    return out, stats


def intrinsic_seed(loc):
    """(focal, ppx, ppy) of the intrinsic group the sequential engine creates for a view resected without one
    (sequential_SfM.cpp:986-987): focal = (K(0,0) + K(1,1)) / 2, the principal point (K(0,2), K(1,2))"""
    if not loc.ok or getattr(loc, "K", None) is None:
        raise ValueError("the view was not resected by localize_uncalibrated")
    K = loc.K
    return (K[0, 0] + K[1, 1]) / 2.0, float(K[0, 2]), float(K[1, 2])


def dlt6(x_norm, X):
    """The six-point solver alone (test hook mvgx_resection_debug_dlt6), one wave per sample. x_norm: (n, 6, 2) NORMALISED pixels, X:
    (n, 6, 3). Returns (P (n, 3, 4) in the normalised space - zeros without a model -, count (n) 0 / 1, ratio (n) of the second smallest
    to the largest singular value, sweeps (n) of the Jacobi iteration)."""
    x_norm = np.ascontiguousarray(x_norm, np.float64).reshape(-1, 6, 2)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 6, 3)
    if len(x_norm) != len(X):
        raise ValueError("x_norm and X differ in length")
    n = len(X)
    P = np.zeros((n, 3, 4))
    info = np.zeros((n, 2))
    count = np.zeros(n, np.int32)
    fn = _capi.lib().mvgx_resection_debug_dlt6
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    _capi.check(fn(x_norm.ctypes.data, X.ctypes.data, n, P.ctypes.data, info.ctypes.data, count.ctypes.data))
    return P, count, info[:, 0].copy(), info[:, 1].astype(np.int32)


def p3p(solver, bearings, X):
    """The minimal solver alone (test hook mvgx_resection_debug_p3p), one lane per sample. bearings, X: (n, 3, 3), three unit bearings and
    three points per sample (one vector per row). Returns (Rt (n, 4, 3, 4), count (n)): up to four [R | t] per sample in the reference's order."""
    bearings = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3, 3)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3, 3)
    if len(bearings) != len(X):
        raise ValueError("bearings and X differ in length")
    n = len(X)
    Rt = np.zeros((n, 4, 3, 4))
    count = np.zeros(n, np.int32)
    fn = _capi.lib().mvgx_resection_debug_p3p
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    _capi.check(fn(int(SOLVERS.get(solver, solver)), bearings.ctypes.data, X.ctypes.data, n, Rt.ctypes.data, count.ctypes.data))
    return Rt, count


def angle_axis(R):
    """the angle-axis vector of a rotation matrix (ceres::RotationMatrixToAngleAxis through the quaternion): the BA scenes' pose layout"""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= 0.0:
        s = math.sqrt(tr + 1.0)
        q = [0.5 * s, (R[2, 1] - R[1, 2]) * 0.5 / s, (R[0, 2] - R[2, 0]) * 0.5 / s, (R[1, 0] - R[0, 1]) * 0.5 / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = [0.0] * 4
        q[i + 1] = 0.5 * s
        q[0] = (R[k, j] - R[j, k]) * 0.5 / s
        q[j + 1] = (R[j, i] + R[i, j]) * 0.5 / s
        q[k + 1] = (R[k, i] + R[i, k]) * 0.5 / s
    sin2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if sin2 > 0.0:
        sin_t = math.sqrt(sin2)
        two_t = 2.0 * (math.atan2(-sin_t, -q[0]) if q[0] < 0.0 else math.atan2(sin_t, q[0]))
        return np.array(q[1:]) * (two_t / sin_t)
    return np.array(q[1:]) * 2.0


def pose_row(loc):
    """(angle-axis | t) of a resected view: the row of "poses" in the flat scene of openmvg_amd.ba / triangulation.triangulate_scene"""
    if not loc.ok:
        raise ValueError("the view was not resected")
    return np.concatenate([angle_axis(loc.R), loc.t])
