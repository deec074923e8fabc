"""Float64 restatement of the reference's relative pose from an essential matrix - the yardstick of the relative-pose tests (TEST
INFRASTRUCTURE). It sits on tests/_triangulation_ref.two_view.

What is restated (paths under src/openMVG of the reference):
  multiview/essential.cpp:79-113             MotionFromEssential (numpy.linalg.svd: LAPACK instead of Eigen's JacobiSVD - the singular
                                             vectors agree up to the sign choices include/mvgx.h describes, so the ORDER of the four
                                             candidates may be permuted 0 <-> 1, 2 <-> 3; counts are compared sorted)
  multiview/motion_from_essential.cpp:20-95  RelativePoseFromEssential: the vote, the first maximum, the ratio of the two largest counts
Besides the result, every pair carries its smallest decision margins: of the in-front test of every triangulated point (the four-norm
comparison of the midpoint method, the ray parameters of the angular methods, the depths of the DLT) and |second / best - ratio|.
"""
import math

import numpy as np

from tests import _triangulation_ref as tref

IDENTITY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
ZERO = (0.0, 0.0, 0.0)


def motion_from_essential(E):
    """-> [(R, t)] x 4 in the reference's order: (R0, t0) (R1, t1) (R0, t1) (R1, t0), t0 = U.col(2), t1 = -t0"""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U[:, 2] *= -1
    if np.linalg.det(Vt) < 0:
        Vt[2] *= -1
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R = (U @ W @ Vt, U @ W.T @ Vt)
    t = (U[:, 2].copy(), -U[:, 2])
    return [(R[0], t[0]), (R[1], t[1]), (R[0], t[1]), (R[1], t[0])]


def in_front_margin(method, R1, t1, x0, x1, X):
    """how far the in-front test of Triangulate2View(method) with the first camera at the origin is from flipping (0 at the edge)"""
    if method == tref.DLT:
        return min(abs(X[2]), abs(tref.to_camera(R1, t1, X)[2]))
    R, t = R1, t1   # AbsoluteToRelative with pose 1 = identity
    Rx0 = tuple(R[i][0] * x0[0] + R[i][1] * x0[1] + R[i][2] * x0[2] for i in range(3))
    if method == tref.IDW_MIDPOINT:
        cp, cq, cr = tref._cross(Rx0, x1), tref._cross(Rx0, t), tref._cross(x1, t)
        pn, qn, rn = (math.sqrt(tref._dot(c, c)) for c in (cp, cq, cr))
        if pn == 0.0:
            return 0.0
        l0 = tuple(rn / pn * v for v in Rx0)
        l1 = tuple(qn / pn * v for v in x1)

        def sq(s0, s1):
            e = tuple(t[i] + s0 * l0[i] + s1 * l1[i] for i in range(3))
            return tref._dot(e, e)
        a, b = sq(1, -1), min(sq(1, 1), sq(-1, -1), sq(-1, 1))
        return abs(a - b) / max(a, b, 1e-300)
    # the angular methods: l0, l1 of Compute3DPoint on the corrected rays - restated through the point they give: xp = t + l0 m0 is X in the
    # second camera's frame, and l1 m1 = xp as well, so the signs of l0 and l1 are those of (xp - t) . Rx0 and xp . x1
    xp = tref.to_camera(R1, t1, X)
    d0 = tuple(xp[i] - t[i] for i in range(3))
    return min(abs(tref._dot(d0, Rx0)) / max(tref._dot(Rx0, Rx0), 1e-300), abs(tref._dot(xp, x1)) / max(tref._dot(x1, x1), 1e-300))


class Result:
    def __init__(self):
        self.ok = False
        self.R, self.t, self.center = np.zeros((3, 3)), np.zeros(3), np.zeros(3)
        self.cheirality = (0, 0, 0, 0)
        self.selected = np.zeros(0, np.uint32)
        self.points = np.zeros((0, 3))
        self.point_margin = math.inf   # smallest in-front margin over every (candidate, correspondence)
        self.ratio_margin = math.inf   # |second / best - ratio|; inf where best = 0


def relative_pose_from_essential(bI, bJ, E, use=None, ratio=0.7, method=tref.IDW_MIDPOINT):
    """RelativePoseFromEssential on one pair: bI / bJ (n, 3), use = positions to vote with (None: all, in order)"""
    bI = np.asarray(bI, np.float64).reshape(-1, 3)
    bJ = np.asarray(bJ, np.float64).reshape(-1, 3)
    use = range(len(bI)) if use is None else [int(u) for u in use]
    res = Result()
    if not np.isfinite(np.asarray(E, np.float64)).all():
        return res
    poses = motion_from_essential(E)
    counts, kept = [], []
    for R, t in poses:
        Rr, tt = tuple(tuple(float(v) for v in row) for row in R), tuple(float(v) for v in t)
        sel, pts = [], []
        for i in use:
            x0, x1 = tuple(float(v) for v in bI[i]), tuple(float(v) for v in bJ[i])
            with np.errstate(all="ignore"):
                try:
                    ok, X = tref.two_view(method, IDENTITY, ZERO, x0, Rr, tt, x1)
                except ZeroDivisionError:
                    ok, X = False, (math.nan,) * 3
            if all(math.isfinite(v) for v in X):
                res.point_margin = min(res.point_margin, in_front_margin(method, Rr, tt, x0, x1, X))
            if ok:
                sel.append(i); pts.append(X)
        counts.append(len(sel)); kept.append((sel, pts))
    res.cheirality = tuple(counts)
    best = int(np.argmax(counts))   # the first maximum
    if counts[best] == 0:
        return res
    s = sorted(counts)
    r = s[-2] / float(s[-1])
    res.ratio_margin = abs(r - ratio)
    # (the reference exports pose and lists before the ratio test and returns false after it; its callers drop such a pair)
    res.ok = r < ratio
    if res.ok:
        res.R, res.t = np.asarray(poses[best][0]), np.asarray(poses[best][1])
        res.center = -res.R.T @ res.t
        res.selected = np.array(kept[best][0], np.uint32)
        res.points = np.array(kept[best][1], np.float64).reshape(-1, 3)
    return res


# ---- the scene family of the tests ----
def rotation(axis_angle):
    return np.array(tref.rotation(axis_angle))


def essential(R, t):
    t = np.asarray(t, np.float64)
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]) @ np.asarray(R, np.float64)


def general_motion(rng):
    """a rotation of 0.1 .. 0.4 rad about a random axis and a unit translation with every component away from zero"""
    axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
    t = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3); t /= np.linalg.norm(t)
    return rotation(axis * rng.uniform(0.1, 0.4)), t


def points_in_front(R, t, n, rng):
    """n points with depth in [2, 8] before the first camera (at the origin) that are before the second camera (R, t) as well"""
    out = []
    while len(out) < n:
        X = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(2, 8)])
        if (R @ X + t)[2] > 1.0:
            out.append(X)
    return np.array(out).reshape(-1, 3)


def bearings(R, t, X):
    """unit bearing vectors of the points in the two cameras (noise-free)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    Y = X @ np.asarray(R).T + np.asarray(t)
    return X / np.linalg.norm(X, axis=1, keepdims=True), Y / np.linalg.norm(Y, axis=1, keepdims=True)


# ---- the cases of the cheirality stage: one pair each, {key, method, ratio, E, bI, bJ, use (None = all in order)} ----
EDGE_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 129)   # around a row of 16 lanes, a wave of 64, and two waves' worth plus one
SUBSET_OF = {63: 40, 129: 77}                      # pairs that are voted on a second time, with a shuffled subset of this length
RATIO_CASES = ((10, 7), (20, 14), (10, 6), (17, 3))   # (m, k): 7 / 10.0 < 0.7 and 14 / 20.0 < 0.7 are false in double -> rejected; the others accepted
SEED = 20261021


def ratio_pair(m, k, rng):
    """m points in front under (R, t) mixed with k points generated in front under (R, -t): both sets satisfy x2^T E x1 = 0 for
    E = [t]x R, the counts of the two candidates with the true rotation are m and k, of the twisted pair 0 and 0"""
    R, t = general_motion(rng)
    a0, b0 = bearings(R, t, points_in_front(R, t, m, rng))
    a1, b1 = bearings(R, -t, points_in_front(R, -t, k, rng))
    order = rng.permutation(m + k)
    return R, t, np.concatenate([a0, a1])[order], np.concatenate([b0, b1])[order], np.flatnonzero(order < m).astype(np.uint32)


def stage_cases():
    """(the geometry is drawn once and shared by the four methods: the fixture stores every input once)"""
    rng = np.random.default_rng([SEED, 0])
    geo = []
    for n in EDGE_LENS:
        R, t = general_motion(rng)
        bI, bJ = bearings(R, t, points_in_front(R, t, n, rng))
        geo.append(dict(key=("edge", n, 0), E=essential(R, t), bI=bI, bJ=bJ, use=None, R=R, t=t))
        if n in SUBSET_OF:
            geo.append(dict(geo[-1], key=("edge", n, 1), use=rng.permutation(n)[:SUBSET_OF[n]].astype(np.uint32)))
    for m, k in RATIO_CASES:
        R, t, bI, bJ, _ = ratio_pair(m, k, rng)
        geo.append(dict(key=("ratio", m, k), E=essential(R, t), bI=bI, bJ=bJ, use=None, R=R, t=t))
    return [dict(g, key=(g["key"][0], method) + g["key"][1:], method=method, ratio=0.7) for method in range(4) for g in geo]


def no_solution_pair():
    """A pure translation along the optical axis, E = [e3]x, and three correspondences that look at the epipole with both cameras
    (x2 = x1 = e3): under every candidate the two rays lie ON the baseline, every cross product of the closed forms is an exact zero
    (the entries of E, of its singular vectors and of the bearings are 0 and +-1: nothing rounds), the ray parameters are 0 / 0 and no
    comparison with a NaN holds; the DLT's design matrix has rank 2 and its null vector is a point at depth 0 or at infinity. Every
    count is 0 under all four methods - the generator of the fixture confirms it on the compiled reference."""
    E = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    b = np.tile(np.array([0.0, 0.0, 1.0]), (3, 1))
    return E, b, b.copy()


# ---- the cases of the robust entry (pinhole): pixels with 0.5 px noise, a share of uniform outliers ----
ROBUST_SETTINGS = ((6.25, 256), (16.0, 4096))   # (initial_residual_tolerance, iterations): Relative_Pose_Engine, the sequential engine
ROBUST_N = (30, 40, 55, 75, 100, 140, 200, 300)
ROBUST_OUTLIERS = (0.0, 0.3, 0.6)
IMAGE_WH, FOCAL = (1000, 1000), 1000.0
K_MATRIX = np.array([[FOCAL, 0.0, 500.0], [0.0, FOCAL, 500.0], [0.0, 0.0, 1.0]])


def robust_pair(n, outliers, rng):
    """-> xI, xJ (n, 2) pixels"""
    R, t = general_motion(rng)
    X = points_in_front(R, t, n, rng)
    Y = X @ R.T + t
    xI = X[:, :2] / X[:, 2:3] * FOCAL + 500.0 + 0.5 * rng.standard_normal((n, 2))
    xJ = Y[:, :2] / Y[:, 2:3] * FOCAL + 500.0 + 0.5 * rng.standard_normal((n, 2))
    bad = rng.permutation(n)[:int(round(outliers * n))]
    xJ[bad] = rng.uniform(0.0, 1000.0, (len(bad), 2))
    return xI, xJ


def robust_cases():
    """24 pairs of 30 .. 300 correspondences with 0, 30 and 60 % outliers, and one of 12 good correspondences (too few: below 13 inliers)"""
    rng = np.random.default_rng([SEED, 7])
    pairs = [robust_pair(n, o, rng) for n in ROBUST_N for o in ROBUST_OUTLIERS] + [robust_pair(12, 0.0, rng)]
    start = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.uint64)
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), start
