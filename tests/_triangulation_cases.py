"""What the emulation and the GPU tests of mvgx_triangulate_tracks share: the comparison with the restatement and its tolerances."""
import numpy as np

from openmvg_amd import triangulation
from tests import _triangulation_ref as ref

# Largest |dX| between the restatement and the compiled reference (tests/test_triangulation_ref_cpu.py prints them; DESIGN.md,
# "Triangulation"), per solver. The device may differ from the restatement by 1000 x that: three orders for its summation grouping,
# fused multiply-adds, f64 division and sqrt sequences and its Jacobi eigen-solver - about 2e-11 on coordinates of order 1.
# (The DLT figure dates from the restatement that took the null vector from LAPACK's SVD; with the two-sided Jacobi iteration it runs now it
# equals the compiled reference bit for bit on those pairs. The figure stays: it is the size of a rounding difference between two correct
# solvers on this family, which is what the rule needs.)
SPREAD = {"closed": 3.6e-15, "dlt": 1.6e-14, "nview": 2.4e-15}
MIN_MARGIN = 1e-6   # guard on the INPUTS: no decision of the restatement, no gap between two hypothesis errors closer than this


def solver_of(mode, n, method, k):
    """which solver produces the point of a track of n observations"""
    if mode == "blind":
        return "closed" if n == 2 else "nview"
    views = n if (n == k) else k   # the all-observations case triangulates the whole track (n == min_required == k)
    if views > 2:
        return "nview"
    return "dlt" if method == ref.DLT else "closed"


def x_tolerance(sc, mode, method, k):
    n = np.diff(np.asarray(sc["track_start"]).astype(np.int64))
    return np.array([1000.0 * SPREAD[solver_of(mode, int(v), method, k)] for v in n])


_CACHE = {}


def reference(name, sc, **kw):
    """the restatement's result for a named case (the name stands for the scene), computed once per process"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = ref.triangulate(*ref.args_of(sc), obs_defined=sc.get("obs_defined"), **kw)
    return _CACHE[key]


def run_device(sc, mode="robust", method=ref.IDW_MIDPOINT, min_required_inliers=3, min_sample_index=3, max_reprojection_error=4.0):
    return triangulation.triangulate_tracks(*ref.args_of(sc), mode=mode, method=method, max_reprojection_error=max_reprojection_error,
                                            min_required_inliers=min_required_inliers, min_sample_index=min_sample_index,
                                            obs_defined=sc.get("obs_defined"))


def subset(sc, tracks):
    """the scene of the named tracks alone (poses and intrinsics stay)"""
    start = np.asarray(sc["track_start"]).astype(np.int64)
    order = np.concatenate([np.arange(start[t], start[t + 1]) for t in tracks] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = dict(sc, track_start=np.concatenate([[0], np.cumsum([start[t + 1] - start[t] for t in tracks])]).astype(np.uint64))
    for k in ("obs_pose", "obs_intr", "obs_xy", "obs_defined", "displaced"):
        if sc.get(k) is not None:
            out[k] = np.asarray(sc[k])[order]
    if "points" in sc:
        out["points"] = np.asarray(sc["points"])[list(tracks)]
    return out


def compare(name, sc, mode="robust", method=ref.IDW_MIDPOINT, min_required_inliers=3, min_sample_index=3, guard=True, unguarded=()):
    """Runs the library (whatever _capi routes to) and the restatement on the scene: decisions equal, every track's X within the
    tolerance of its solver. Returns (device result, restatement, largest |dX|).
    guard: the guard on the inputs - True: decision margins and hypothesis gaps; "gap": the gaps alone (scenes whose two-view samples
    can share a pose: such a sample's point is the camera centre to rounding, its cheirality dot product is rounding, and it is rejected
    on its residuals). unguarded: tracks that are degenerate ON PURPOSE - the guard is taken from the restatement of the other tracks."""
    kw = dict(mode=mode, method=method, min_required_inliers=min_required_inliers, min_sample_index=min_sample_index)
    want = reference(name, sc, **kw)
    guarded = want
    if len(unguarded):
        guarded = reference(name + "/guarded", subset(sc, [t for t in range(len(want.ok)) if t not in set(unguarded)]), **kw)
    print(f"{name} {kw}: restatement margin {guarded.margin:.3g}, gap {guarded.gap:.3g}, kept {int(want.ok.sum())}/{len(want.ok)}")
    if guard:
        assert guard == "gap" or guarded.margin >= MIN_MARGIN, "the inputs sit on a decision boundary: choose another seed"
        assert guarded.gap >= MIN_MARGIN, "two hypothesis errors are too close to tell apart: choose another seed"
    X, ok, inl, stats = run_device(sc, **kw)
    dev = float(np.abs(X - want.X).max()) if len(X) else 0.0
    print(f"{name}: largest |dX| device vs restatement {dev:.3g}")
    assert np.array_equal(ok, want.ok)
    assert np.array_equal(inl[: len(want.inl)], want.inl)
    assert stats.n_hypotheses == want.n_hypotheses
    assert stats.n_tracks == len(ok) and stats.n_kept == int(want.ok.sum()) and stats.n_inlier_obs == int(want.inl.sum())
    assert np.all(X[~want.ok] == 0.0)
    tol = x_tolerance(sc, mode, method, min_sample_index)
    assert np.all(np.abs(X - want.X).max(axis=1) <= tol), (np.abs(X - want.X).max(axis=1) / tol).max()
    return (X, ok, inl, stats), want, dev


def mixed_lengths(n_tracks, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, n_tracks)


def expected_hypotheses(sc, need, k):
    """the rule of tri_plan: 2 n per track that reaches the loop (n >= need, n >= k, and not the all-observations case n == need == k)"""
    n = np.diff(np.asarray(sc["track_start"]).astype(np.int64))
    loop = (n >= need) & (n >= k) & ~((need == k) & (n == need))
    return int(2 * n[loop].sum())


# ---- scenes both test files use ----
ROBUST_FORMS = [(2, 2), (3, 2), (3, 3)]   # (min_required_inliers, min_sample_index) of the reference's callers
OTHER_FORMS = [(1, 2), (2, 3), (4, 3), (5, 2)]
# group boundaries of the robust kernel: 16-lane groups up to 8 observations, LDS records and the inlier mask up to 64, rounds of 64 hypotheses above 32
BOUNDARY_LENGTHS = [2, 3, 8, 9, 32, 33, 63, 64, 65]
ALL_METHODS = (ref.DLT, ref.L1_ANGULAR, ref.LINF_ANGULAR, ref.IDW_MIDPOINT)


def robust_methods(k):
    return list(ALL_METHODS) if k == 2 else [ref.IDW_MIDPOINT]


def with_undefined(sc, tracks, seed=5, poison=False):
    """One observation of each named track becomes a view without pose or intrinsic. Its indices are made unusable on purpose
    (0xFFFFFFFF: the emulation, where a read through them is caught on the host), or - poison - point at an extra pose row and an extra
    intrinsic row of a valid model, both all NaN: an unguarded read on a device then shows as a wrong decision, not as a memory fault."""
    sc = dict(sc)
    rng = np.random.default_rng(seed)
    sc["obs_defined"] = np.ones(len(sc["obs_pose"]), np.uint8)
    sc["obs_pose"] = sc["obs_pose"].copy(); sc["obs_intr"] = sc["obs_intr"].copy()
    bad_pose = bad_intr = 0xFFFFFFFF
    if poison:
        bad_pose, bad_intr = len(sc["poses"]), len(sc["intrinsics"])
        sc["poses"] = np.concatenate([sc["poses"], np.full((1, 6), np.nan)])
        sc["intrinsics"] = np.concatenate([sc["intrinsics"], np.full((1, 8), np.nan)])
        sc["intr_model"] = np.concatenate([sc["intr_model"], [ref.PINHOLE]]).astype(np.int32)
    for t in tracks:
        lo, hi = int(sc["track_start"][t]), int(sc["track_start"][t + 1])
        o = int(rng.integers(lo, hi))
        sc["obs_defined"][o] = 0
        sc["obs_pose"][o] = bad_pose; sc["obs_intr"][o] = bad_intr
    return sc


def behind_track(model):
    """three adjacent cameras of the ring and a point BEHIND them (off the middle camera's axis): the lines meet there, the rays of a
    perspective camera do not. A spherical camera sees it like any other point."""
    from openmvg_amd import synth
    sc = ref.scene(8, [3], model=model, seed=77, noise=0.0)
    sc["obs_pose"] = np.array([0, 1, 2], np.uint32)
    R = synth._rodrigues(sc["poses"][1, :3])[0]
    centre = -R.T @ sc["poses"][1, 3:6]
    sc["points"] = (1.5 * centre + (0.3, 0.2, 0.1))[None]
    sc["obs_xy"] = synth.project(model, np.repeat(sc["intrinsics"], 3, 0), sc["poses"][:3], np.repeat(sc["points"], 3, 0))
    return sc


def degenerate_pairs():
    """Two-view tracks without a solution, beside five ordinary ones (tracks 0 - 4, the guarded ones). Every degenerate track is built
    from numbers whose degeneracy is EXACT in floating point (identity rotations, centres at the origin, a pixel at the principal point),
    so that what the reference computes is a zero or a NaN and not a rounding error of either sign - except 'parallel-generic', whose
    cross product x * x is exactly zero only where the two products of each component round alike, i.e. without a fused multiply-add.
    Returns (scene, {name: track})."""
    sc = ref.scene(8, [2] * 5, seed=1234, noise=0.5)
    f, cx, cy = sc["intrinsics"][0, :3]
    poses, obs_pose, xy, names = list(sc["poses"]), list(sc["obs_pose"]), list(sc["obs_xy"]), {}

    def add(name, pose0, pose1, xy0, xy1):
        names[name] = len(obs_pose) // 2
        for pose, x in ((pose0, xy0), (pose1, xy1)):
            if isinstance(pose, int):
                obs_pose.append(pose)
            else:
                obs_pose.append(len(poses)); poses.append(np.asarray(pose, np.float64))
            xy.append(x)

    front = [0, 0, 0, 0, 0, 5.0]   # identity rotation, centre (0, 0, -5)
    add("shared-pose", front, len(poses), (620.0, 410.0), (380.0, 590.0))          # one pose row, two pixels: zero baseline
    add("shared-pose-same-pixel", front, len(poses), (620.0, 410.0), (620.0, 410.0))
    add("pure-rotation", [0.02, -0.03, 0.01, 0, 0, 0], [-0.04, 0.05, 0.02, 0, 0, 0], (620.0, 410.0), (380.0, 590.0))   # both centres at the origin
    add("parallel-clean", front, [0, 0, 0, 1.0, 0, 5.0], (cx, cy), (cx, cy))       # both rays along +z, baseline along x
    add("parallel-generic", front, [0, 0, 0, 0.7, -0.4, 5.2], (623.17, 408.61), (623.17, 408.61))
    # the point IS the centre of the first camera (the origin); the second, at (0, 0, -5), sees it at its principal point
    add("point-at-centre", [0, 0, 0, 0, 0, 0], front, (620.0, 410.0), (cx, cy))
    n = len(obs_pose)
    out = dict(sc, poses=np.stack(poses), track_start=(2 * np.arange(n // 2 + 1)).astype(np.uint64), obs_pose=np.array(obs_pose, np.uint32),
               obs_intr=np.zeros(n, np.uint32), obs_xy=np.array(xy, np.float64))
    out.pop("points"); out.pop("displaced")
    return out, names


# ---- the form edges: one body per case, run under the emulation and on the device (poison: how a view without pose is marked) ----
def check_group_boundaries(need, k, poison):
    """every length at which the kernel changes form, the all-observations case (n == need == k, the first tracks) and views without pose"""
    sc = ref.scene(72, BOUNDARY_LENGTHS * 2, seed=300 + 10 * need + k)
    sc = with_undefined(sc, [12, 13, 15, 17], poison=poison)   # tracks of 9, 32, 63 and 65 observations
    for method in robust_methods(k):
        (_, ok, inl, _), want, _ = compare(f"robust-boundaries-{need}-{k}", sc, method=method, min_required_inliers=need, min_sample_index=k)
        assert ok.sum() >= 14
        assert not inl[sc["displaced"]].any()   # no displaced observation ends up an inlier


def check_blind_rejections(model, poison):
    sc = with_undefined(ref.scene(8, [2, 3, 6, 6], model=model, seed=60 + model), [1, 2], poison=poison)
    (_, ok, _, _), _, _ = compare(f"blind-undefined-{model}", sc, mode="blind")
    assert list(ok[[1, 2]]) == [False, False] and ok[3]
    (_, ok, _, _), _, _ = compare(f"blind-behind-{model}", behind_track(model), mode="blind")
    assert ok[0] == (model == ref.SPHERICAL)


def check_robust_behind(model):
    (_, ok, _, _), _, _ = compare(f"robust-behind-{model}", behind_track(model))
    assert ok[0] == (model == ref.SPHERICAL)


def check_views_without_pose(poison):
    """the small, wave and global classes and the blind kernel: tracks of 6, 9, 32, 63 and 65 observations, one view of each without pose,
    beside the same lengths whole"""
    lengths = [6, 9, 32, 63, 65]
    sc = with_undefined(ref.scene(72, lengths * 2, seed=1300), range(5), seed=6, poison=poison)
    (_, ok, _, _), _, _ = compare("undefined-blind", sc, mode="blind")
    assert not ok[:5].any() and ok[5:].all()   # blind: a track with such a view is not triangulated at all (:63-64)
    for need, k in ((3, 3), (2, 2)):
        (_, ok, inl, _), _, _ = compare("undefined-robust", sc, min_required_inliers=need, min_sample_index=k)
        assert ok.all()                         # robust: the samples that avoid the view still triangulate the track
        assert not inl[sc["obs_defined"] == 0].any()


def check_mixed_cameras():
    """eight intrinsic rows of all six models, one per pose: the views of a track differ in model and in intrinsic row"""
    short = ref.scene(16, mixed_lengths(48, 2, 12, seed=51), seed=1401, mixed=True)
    long_ = ref.scene(72, mixed_lengths(6, 33, 70, seed=52), seed=1402, mixed=True)
    for name, sc in (("mixed-short", short), ("mixed-long", long_)):
        start = sc["track_start"].astype(np.int64)
        per_track = [len(set(sc["intr_model"][sc["obs_intr"][start[t]:start[t + 1]]])) for t in range(len(start) - 1)]
        assert np.mean(per_track) >= 2 and len(set(sc["obs_intr"])) == 8   # the scene is what it claims to be
        (_, ok, _, _), _, _ = compare(name, sc, mode="blind")
        assert ok.mean() > 0.8
        for need, k in ((3, 3), (2, 2)):
            (_, ok, inl, _), _, _ = compare(name, sc, min_required_inliers=need, min_sample_index=k)
            n = np.diff(start)
            assert ok[n >= 3].mean() > 0.8 and not inl[sc["displaced"]].any()


def check_ragged_groups():
    """1, 2, 3 and 5 tracks of the small class (four 16-lane groups per workgroup: the lanes of a group without a track), one track alone of
    each class (all-observations, small, wave with one round and with two, global), and a call with one class only"""
    for count in (1, 2, 3, 5):
        sc = ref.scene(8, [5, 7, 4, 8, 6][:count], seed=1500 + count)
        (_, ok, _, stats), _, _ = compare(f"ragged-{count}", sc)
        assert ok.all() and stats.n_hypotheses == expected_hypotheses(sc, 3, 3)
    for n in (3, 6, 20, 40, 66):
        sc = ref.scene(72, [n], seed=1510 + n)
        (_, ok, _, _), _, _ = compare(f"alone-{n}", sc)
        assert ok.all()
        if n == 3:   # the all-observations kernel in its DLT form on three views: the method plays no part, the N-view solver does
            (Xd, ok, _, _), _, _ = compare(f"alone-{n}", sc, method=ref.DLT)
            assert ok.all()
    sc = ref.scene(72, [40, 33, 64, 50, 37], seed=1520)
    (_, ok, _, _), _, _ = compare("wave-class-only", sc)
    assert ok.all()


def check_other_caller_form(need, k):
    sc = ref.scene(12, mixed_lengths(40, 2, 12, seed=61), seed=1600 + 10 * need + k)
    for method in robust_methods(k):
        (_, ok, _, stats), want, _ = compare(f"form-{need}-{k}", sc, method=method, min_required_inliers=need, min_sample_index=k)
        n = np.diff(sc["track_start"].astype(np.int64))
        assert stats.n_hypotheses == expected_hypotheses(sc, need, k) and not ok[(n < need) | (n < k)].any()
        assert ok[n >= max(need, k) + 1].mean() > 0.8


def run_capi(sc, first_track, fill, **options):
    """mvgx_triangulate_tracks on the tracks from first_track on, the observation arrays passed WHOLE (track_start[0] > 0), obs_inlier
    filled with `fill` before the call -> (X, ok, obs_inlier bytes, stats)"""
    import ctypes as C
    from openmvg_amd import _capi
    a = dict(poses=np.ascontiguousarray(sc["poses"], np.float64), intrinsics=np.ascontiguousarray(sc["intrinsics"], np.float64),
             intr_model=np.ascontiguousarray(sc["intr_model"], np.int32), track_start=np.ascontiguousarray(sc["track_start"][first_track:], np.uint64),
             obs_pose=np.ascontiguousarray(sc["obs_pose"], np.uint32), obs_intr=np.ascontiguousarray(sc["obs_intr"], np.uint32),
             obs_xy=np.ascontiguousarray(sc["obs_xy"], np.float64))
    n_tracks = len(a["track_start"]) - 1
    X, ok, inl = np.zeros((n_tracks, 3)), np.zeros(n_tracks, np.uint8), np.full(len(a["obs_pose"]), fill, np.uint8)
    opt = triangulation.default_options(**options)
    stats = _capi.TriangulateStats()
    _capi.check(_capi.lib().mvgx_triangulate_tracks(
        -1, a["poses"].ctypes.data, len(a["poses"]), a["intrinsics"].ctypes.data, a["intr_model"].ctypes.data, len(a["intrinsics"]),
        a["track_start"].ctypes.data, n_tracks, a["obs_pose"].ctypes.data, a["obs_intr"].ctypes.data, a["obs_xy"].ctypes.data, None, C.byref(opt),
        X.ctypes.data, ok.ctypes.data, inl.ctypes.data, C.byref(stats)))
    return X, ok.astype(bool), inl, stats


def check_offset_observation_arrays():
    """a call on the tracks from the 8th on, with the arrays of the whole scene: the slice of the whole scene's result, and not a byte of
    obs_inlier before the first track written"""
    from openmvg_amd import _capi
    sc = ref.scene(72, list(mixed_lengths(30, 2, 12, seed=71)) + [40, 66], seed=1700, mixed=True)
    first = 7
    base = int(sc["track_start"][first])
    for options in (dict(mode=_capi.MVGX_TRI_BLIND), dict(mode=_capi.MVGX_TRI_ROBUST), dict(mode=_capi.MVGX_TRI_ROBUST, min_required_inliers=2, min_sample_index=2)):
        X, ok, inl, stats = run_capi(sc, 0, 0xAA, **options)
        Xs, oks, inls, stats_s = run_capi(sc, first, 0xAA, **options)
        assert ok.sum() >= 20 and not np.any(inl == 0xAA)
        assert np.array_equal(Xs, X[first:]) and np.array_equal(oks, ok[first:]) and np.array_equal(inls[base:], inl[base:])
        assert np.all(inls[:base] == 0xAA)
        assert stats_s.n_kept == int(ok[first:].sum()) and stats_s.n_inlier_obs == int(inl[base:].sum())


# Degenerate tracks on which the reference's own result is not a decision but a rounding error, per method: there only the form of the
# output is checked. Parallel rays of generic numbers: the midpoint's `pn == 0` guard rejects them; the DLT's null vector is a point at
# infinity whose last coordinate is rounding, the angular methods' z = m1 x m0 likewise. One pose, one pixel: D has rank 2 and every point
# of the ray is a null vector - LAPACK returns one of them, in front of the camera and with residual 0.
FORM_ONLY = {"parallel-generic": (ref.DLT, ref.L1_ANGULAR, ref.LINF_ANGULAR), "shared-pose-same-pixel": (ref.DLT,)}


def check_degenerate_pairs():
    """every method, blind and robust (2, 2), on two-view tracks without a solution: the decisions of the restatement (rejected, by both),
    zeros for every rejected track, no NaN and no infinity in any output"""
    sc, names = degenerate_pairs()
    degenerate = sorted(names.values())
    runs = [("blind", None, dict(mode="blind"))] + [(f"robust-{m}", m, dict(method=m, min_required_inliers=2, min_sample_index=2)) for m in ALL_METHODS]
    for label, method, kw in runs:
        form_only = [names[n] for n, methods in FORM_ONLY.items() if method in methods]
        tracks = [t for t in range(len(sc["track_start"]) - 1) if t not in form_only]
        (X, ok, inl, _), want, _ = compare(f"degenerate-{label}", subset(sc, tracks), unguarded=[i for i, t in enumerate(tracks) if t in degenerate], **kw)
        assert np.isfinite(X).all()
        assert ok[:5].all() and not ok[5:].any() and not want.ok[5:].any()
        if form_only:
            X, ok, inl, _ = run_device(subset(sc, [0] + form_only), **kw)
            assert np.isfinite(X).all() and np.all(X[~ok] == 0.0) and ok[0]


def check_samples_sharing_a_pose(need, k):
    """tracks of 9 - 12 observations on 8 poses: some two-view samples are two views of ONE pose (zero baseline)"""
    # (seed 1803 gave a gap of 8.9e-7 with the L-infinity method in the (3, 2) form, below the guard on the inputs, and was replaced)
    sc = ref.scene(8, mixed_lengths(40, 9, 12, seed=81), seed={2: 1802, 3: 1813}[need])
    for method in ALL_METHODS:
        (X, ok, _, _), _, _ = compare(f"shared-pose-samples-{need}-{k}", sc, method=method, min_required_inliers=need, min_sample_index=k, guard="gap")
        assert ok.sum() >= 36 and np.isfinite(X).all()
