"""50-digit restatement of the reference's relative pose from an essential matrix - the yardstick of the hard-case tests of the
cheirality stage (TEST INFRASTRUCTURE). Where tests/_relative_pose_ref.py restates the reference in float64 on LAPACK's SVD (a third
rounding of the same thing), this module computes what the reference's FORMULATIONS give in exact arithmetic, every input (the entries
of E, the bearing vectors) taken as the exact value of its double. It sits on tests/_triangulation_truth.py.

  MotionFromEssential (multiview/essential.cpp:79-113)   the singular triplets of E from the symmetric eigenproblem of E^T E, u_i = E v_i
                     / sigma_i for the two large ones; u3 = u1 x u2 and v3 = v1 x v2 are the unit vectors that make both determinants +1
                     (the third column of an orthogonal matrix of determinant +1 IS the cross product of the first two); R in {U W V^T,
                     U W^T V^T}, t = +-u3. Where sigma_1 and sigma_2 agree to more than 40 digits, the eigenvectors are an arbitrary basis
                     of their plane: the rotations are formed a second time from that basis turned by one radian, and the module asserts
                     that both agree to 40 digits (it is the combination u2 v1^T - u1 v2^T that is determined, not its factors).
  RelativePoseFromEssential (multiview/motion_from_essential.cpp:20-95)   Triangulate2View(method) of every listed correspondence under
                     each candidate (the closed forms and the DLT of _triangulation_truth), the first maximum, second / best < ratio in
                     double arithmetic; the decision margins of tests/_relative_pose_ref.Result, at 50 digits.
The order of the four candidates is this module's own (it follows mp.eigsy); compare the winner, and the counts sorted.
"""
import math

import numpy as np
from mpmath import mp, mpf

from tests import _triangulation_truth as tt

DPS = 50
SOLVER_OF = {0: "dlt", 1: "l1", 2: "linf", 3: "midpoint"}   # ETriangulationMethod
EQUAL_DIGITS, BASIS_TURN = 40, 1   # sigma_1 = sigma_2 to this many digits: any basis serves; the second basis is the first turned by 1 rad


class NoMotion(Exception):
    """E has no two non-zero singular values (the zero matrix, rank one) or is not finite"""


def _outer_terms(u1, u2, v1, v2):
    u3, v3 = tt._cross(u1, u2), tt._cross(v1, v2)
    A = [[u2[i] * v1[j] - u1[i] * v2[j] for j in range(3)] for i in range(3)]
    B = [[u3[i] * v3[j] for j in range(3)] for i in range(3)]
    return [[B[i][j] + A[i][j] for j in range(3)] for i in range(3)], [[B[i][j] - A[i][j] for j in range(3)] for i in range(3)], u3


def _turned(E, v1, v2, angle):
    """the rotations and u3 from the basis (v1, v2) of the plane of the two large singular values turned by `angle`"""
    c, s = mp.cos(angle), mp.sin(angle)
    w = [[c * v1[i] + s * v2[i] for i in range(3)], [-s * v1[i] + c * v2[i] for i in range(3)]]
    u = [tt._normalized([tt._dot(E[i], v) for i in range(3)]) for v in w]
    return _outer_terms(u[0], u[1], w[0], w[1])


def motion_from_essential(E, report=None):
    """E (9 or 3 x 3 doubles) -> (R0, R1, u3) in mpf: the candidates are (R0, u3) (R1, -u3) (R0, -u3) (R1, u3). Call inside
    mp.workdps(DPS). report: a dict that receives `equal` (sigma_1 = sigma_2 to EQUAL_DIGITS digits) and `basis_error` (the difference of
    the two bases' rotations, where the check ran)."""
    E = [[mpf(float(v)) for v in row] for row in np.asarray(E, np.float64).reshape(3, 3)]
    if not all(mp.isfinite(v) for row in E for v in row):
        raise NoMotion("not finite")
    big = max(abs(v) for row in E for v in row)
    if big == 0:
        raise NoMotion("zero")
    E = [[v / big for v in row] for row in E]   # (the decomposition is scale-free; mp's exponents are unbounded, this only keeps the numbers readable)
    lam, Q = mp.eigsy(mp.matrix([[sum(E[k][i] * E[k][j] for k in range(3)) for j in range(3)] for i in range(3)]))
    order = sorted(range(3), key=lambda i: -lam[i])
    s1, s2 = mp.sqrt(max(lam[order[0]], 0)), mp.sqrt(max(lam[order[1]], 0))
    if s2 <= mpf(10) ** (-DPS // 2) * s1:
        raise NoMotion("rank one")
    v1, v2 = ([Q[i, order[k]] for i in range(3)] for k in range(2))
    # (u_i = E v_i / sigma_i = (E v_i).normalized(); E v_1 and E v_2 are orthogonal because v_1 and v_2 are eigenvectors of E^T E)
    R0, R1, u3 = _turned(E, v1, v2, mpf(0))
    equal = abs(s1 - s2) <= mpf(10) ** (-EQUAL_DIGITS) * s1
    if report is not None:
        report["equal"] = bool(equal)
    if equal:
        S0, S1, w3 = _turned(E, v1, v2, mpf(BASIS_TURN))
        err = max(max(abs(R0[i][j] - S0[i][j]), abs(R1[i][j] - S1[i][j])) for i in range(3) for j in range(3))
        err = max(err, max(abs(u3[i] - w3[i]) for i in range(3)))
        if report is not None:
            report["basis_error"] = float(err)
        assert err < mpf(10) ** (-EQUAL_DIGITS), ("the rotations depend on the basis of the singular plane", float(err))
    return R0, R1, u3


def _in_front_margin(solver, R, t, x0, x1, X):
    """_relative_pose_ref.in_front_margin at 50 digits (pose 1 = the identity at the origin)"""
    xp = tt._to_camera(R, t, X)
    if solver == "dlt":
        return min(abs(X[2]), abs(xp[2]))
    Rx0 = [tt._dot(R[i], x0) for i in range(3)]
    if solver == "midpoint":
        cp, cq, cr = tt._cross(Rx0, x1), tt._cross(Rx0, t), tt._cross(x1, t)
        pn, qn, rn = (mp.sqrt(tt._dot(c, c)) for c in (cp, cq, cr))
        l0, l1 = [rn / pn * v for v in Rx0], [qn / pn * v for v in x1]

        def sq(s0, s1):
            e = [t[i] + s0 * l0[i] + s1 * l1[i] for i in range(3)]
            return tt._dot(e, e)
        return tt._relative(sq(1, -1), min(sq(1, 1), sq(-1, -1), sq(-1, 1)))
    d0 = [xp[i] - t[i] for i in range(3)]
    return min(abs(tt._dot(d0, Rx0)) / tt._dot(Rx0, Rx0), abs(tt._dot(xp, x1)) / tt._dot(x1, x1))


class Result:
    """as _relative_pose_ref.Result; R, t, center and points are the 50-digit values rounded to double"""

    def __init__(self):
        self.ok = False
        self.R, self.t, self.center = np.zeros((3, 3)), np.zeros(3), np.zeros(3)
        self.cheirality = (0, 0, 0, 0)
        self.selected = np.zeros(0, np.uint32)
        self.points = np.zeros((0, 3))
        self.point_margin = math.inf   # smallest in-front margin over every (candidate, correspondence)
        self.ratio_margin = math.inf   # |second / best - ratio|; inf where best = 0
        self.equal_singular_values = False


def relative_pose_from_essential(bI, bJ, E, use=None, ratio=0.7, method=3):
    """RelativePoseFromEssential on one pair: bI / bJ (n, 3), use = positions to vote with (None: all, in order; repeats are voted on,
    and listed, as often as they appear)"""
    bI = np.asarray(bI, np.float64).reshape(-1, 3)
    bJ = np.asarray(bJ, np.float64).reshape(-1, 3)
    use = range(len(bI)) if use is None else [int(u) for u in use]
    solver = SOLVER_OF[int(method)]
    res = Result()
    with mp.workdps(DPS):
        report = {}
        try:
            R0, R1, u3 = motion_from_essential(E, report)
        except NoMotion:
            return res
        res.equal_singular_values = report["equal"]
        minus = [-v for v in u3]
        poses = [(R0, u3), (R1, minus), (R0, minus), (R1, u3)]
        eye = ([[mpf(1), mpf(0), mpf(0)], [mpf(0), mpf(1), mpf(0)], [mpf(0), mpf(0), mpf(1)]], [mpf(0)] * 3)
        bs = {i: (tt._vec(bI[i]), tt._vec(bJ[i])) for i in set(use)}
        counts, kept, margin = [], [], mpf("inf")
        for R, t in poses:
            sel, pts = [], []
            for i in use:
                x0, x1 = bs[i]
                try:
                    if solver == "dlt":
                        ok, X, _ = tt._dlt([eye, (R, t)], [x0, x1])
                    else:
                        ok, X, _ = tt._closed(solver, [eye, (R, t)], [x0, x1])
                    margin = min(margin, _in_front_margin(solver, R, t, x0, x1, X))
                except ZeroDivisionError:   # rays on the baseline: 0 / 0 in the reference, no comparison with a NaN holds
                    ok, margin = False, mpf(0)
                if ok:
                    sel.append(i); pts.append([float(v) for v in X])
            counts.append(len(sel)); kept.append((sel, pts))
        res.cheirality = tuple(counts)
        res.point_margin = float(margin)
        best = max(range(4), key=lambda k: (counts[k], -k))   # the first maximum
        if counts[best] == 0:
            return res
        s = sorted(counts)
        r = s[-2] / float(s[-1])
        res.ratio_margin = abs(r - ratio)
        res.ok = r < ratio
        if res.ok:
            R, t = poses[best]
            res.R = np.array([[float(v) for v in row] for row in R])
            res.t = np.array([float(v) for v in t])
            res.center = np.array([float(-(R[0][j] * t[0] + R[1][j] * t[1] + R[2][j] * t[2])) for j in range(3)])
            res.selected = np.array(kept[best][0], np.uint32)
            res.points = np.array(kept[best][1], np.float64).reshape(-1, 3)
    return res
