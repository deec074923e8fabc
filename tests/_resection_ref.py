"""Float64 restatement of the reference's robust resection - the yardstick of the resection tests (TEST INFRASTRUCTURE).

What is restated (paths under src/openMVG of the reference):
  multiview/solver_resection_p3p_ding.cpp:33-325        P3PSolver_Ding
  multiview/solver_resection_p3p_nordberg.cpp:31-454    P3PSolver_Nordberg (root2real: the .hpp, :22-38)
  sfm/pipelines/localization/SfM_Localizer.cpp:31-343   ACKernelAdaptorResection_Intrinsics, SfM_Localizer::Localize
  robust_estimation/robust_estimator_ACRansac.hpp:58-116, :257-304, :326-489   logcombi tables, the exhaustive NFA, the a-contrario loop
  robust_estimation/rand_sampling.hpp:71-100            UniformSample on the pool
  multiview/projection.cpp:40-132                       KRt_From_P
The generator and its bounded draw come from tests/_triangulation_ref.py. Solver scalars are Python floats (IEEE double, one rounding per
operation, the reference's order); residuals and the NFA scan are numpy float64, one rounding per elementwise operation; the logcombi
tables are float32 running sums as the reference's.

Besides its result a run returns its DECISION MARGIN: the smallest relative gap over the comparisons whose outcome changes what the loop
does next or returns (NFA against minNFA, the winning k against its runner-up in an event model, minNFA against 0, the sorted residuals
next to the chosen k, the solvers' branch tests). A device run may differ from this restatement where that margin is below the
arithmetic's spread; such problems are left out of the parity comparison (tests/_resection_cases.py).
"""
import math

import numpy as np

from tests import _triangulation_ref as tri

PINHOLE, RADIAL3, SPHERICAL = tri.PINHOLE, tri.RADIAL3, tri.SPHERICAL
NORDBERG, DING = 3, 4
FLT_EPS = float(np.finfo(np.float32).eps)
LOGALPHA0 = math.log10(math.pi)
# The three points of a sample fit their own model: their residuals are what rounding leaves of an exact zero (1e-13 px here, against the
# 0.5 px of the inputs' noise), and their order at the head of the sorted list - which becomes the order of the sampling pool - is a
# property of the arithmetic, not of the data: a build with fused multiply-adds or another libm orders them differently. A run is
# DECIDED as long as no such point has been drawn from the pool again; from the first iteration that draws one (Run.undecided_at) two
# correct implementations may run different sample sequences. Residuals (in pixels) below this bound count as such noise.
UNORDERED_BELOW_PX = 1e-6


class Margin:
    """the smallest relative gap seen, and where"""

    def __init__(self):
        self.value = math.inf
        self.where = None

    def gap(self, a, b, where, scale=None):
        """the comparison of a with b"""
        s = max(abs(a), abs(b)) if scale is None else scale
        if not (s > 0.0) or not math.isfinite(s):
            return
        g = abs(a - b) / s
        if g < self.value:
            self.value, self.where = g, where


# ---- the solvers ----
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _neg(a):
    return (-a[0], -a[1], -a[2])


def _scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _div(a, b):
    """IEEE division: infinities and NaNs instead of exceptions"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else math.nan


def root2real(b, c, mg, br):
    v = b * b - 4.0 * c
    mg.gap(b * b, 4.0 * c, "root2real v <= 0")
    if v <= 0.0 or v != v:
        if v != v:
            return False, math.nan, math.nan
        return v >= 0.0, -0.5 * b, -0.5 * b
    y = math.sqrt(v)
    br.add("root2real b < 0" if b < 0.0 else "root2real b >= 0")
    if b < 0.0:
        return True, 0.5 * (-b + y), 0.5 * (-b - y)
    return True, _div(2.0 * c, -b + y), _div(2.0 * c, -b - y)


def _frame(c0, c1):
    """rows of [c0 c1 c0 x c1]^-1 by cofactors"""
    c2 = _cross(c0, c1)
    r0, r1, r2 = _cross(c1, c2), _cross(c2, c0), _cross(c0, c1)
    inv_det = _div(1.0, _dot(c0, r0))
    return _scale(r0, inv_det), _scale(r1, inv_det), _scale(r2, inv_det)


def _pose(frame, X0, v1, v2, base):
    v3 = _cross(v1, v2)
    i0, i1, i2 = frame
    R = [[v1[r] * i0[c] + v2[r] * i1[c] + v3[r] * i2[c] for c in range(3)] for r in range(3)]
    t = [base[r] - (R[r][0] * X0[0] + R[r][1] * X0[1] + R[r][2] * X0[2]) for r in range(3)]
    return np.array([R[r] + [t[r]] for r in range(3)])


def _ding_refine(l1, l2, l3, a12, a13, a23, b12, b13, b23, mg):
    for _ in range(5):
        r1 = (l1 * l1 - 2.0 * l1 * l2 * b12 + l2 * l2 - a12)
        r2 = (l1 * l1 - 2.0 * l1 * l3 * b13 + l3 * l3 - a13)
        r3 = (l2 * l2 - 2.0 * l2 * l3 * b23 + l3 * l3 - a23)
        s = abs(r1) + abs(r2) + abs(r3)
        mg.gap(s, 1e-10, "ding refine stop", scale=1e-10)
        if s < 1e-10:
            return l1, l2, l3
        x11, x12 = l1 - l2 * b12, l2 - l1 * b12
        x21, x23 = l1 - l3 * b13, l3 - l1 * b13
        x32, x33 = l2 - l3 * b23, l3 - l2 * b23
        detJ = _div(0.5, x11 * x23 * x32 + x12 * x21 * x33)
        l1, l2, l3 = (l1 + (-x23 * x32 * r1 - x12 * x33 * r2 + x12 * x23 * r3) * detJ,
                      l2 + (-x21 * x33 * r1 + x11 * x33 * r2 - x11 * x23 * r3) * detJ,
                      l3 + (x21 * x32 * r1 - x11 * x32 * r2 - x12 * x21 * r3) * detJ)
    return l1, l2, l3


def _cubic_single_real(c2, c1, c0, mg, br):
    a = c1 - c2 * c2 / 3.0
    b = (2.0 * c2 * c2 * c2 - 9.0 * c2 * c1) / 27.0 + c0
    c = b * b / 4.0 + a * a * a / 27.0
    mg.gap(b * b / 4.0, -(a * a * a / 27.0), "cubic c sign")
    if c != 0:
        if c > 0:
            br.add("cubic c > 0")
            c = math.sqrt(c)
            b *= -0.5
            return True, np.cbrt(b + c).item() + np.cbrt(b - c).item() - c2 / 3.0
        br.add("cubic c < 0")
        c = 3.0 * b / (2.0 * a) * _sqrt(-3.0 / a)
        ac = math.acos(c) if -1.0 <= c <= 1.0 else math.nan
        return False, 2.0 * _sqrt(-a / 3.0) * math.cos(ac / 3.0) - c2 / 3.0
    br.add("cubic c == 0")
    return False, -c2 / 3.0 + ((3.0 * b / a) if a != 0 else 0)


def p3p_ding(bear, X, mg=None, br=None):
    """bear, X: three vectors each. Returns the list of [R | t] (3 x 4 arrays) in the reference's order."""
    mg = Margin() if mg is None else mg
    br = set() if br is None else br
    X0, X1, X2 = (tuple(float(v) for v in X[i]) for i in range(3))
    x0, x1, x2 = (tuple(float(v) for v in bear[i]) for i in range(3))
    X01, X02, X12 = _sub(X0, X1), _sub(X0, X2), _sub(X1, X2)
    a01, a02, a12 = _dot(X01, X01), _dot(X02, X02), _dot(X12, X12)
    mg.gap(a01, a02, "ding a01 > a02")
    if a01 > a02:
        mg.gap(a01, a12, "ding a01 > a12")
        if a01 > a12:
            br.add("ding swap 0-2")
            X0, X2 = X2, X0
            x0, x2 = x2, x0
            a01, a12 = a12, a01
            X01 = _neg(X12)
            X02 = _neg(X02)
        else:
            br.add("ding no swap (a01 > a02)")
    else:
        mg.gap(a02, a12, "ding a02 > a12")
        if a02 > a12:
            br.add("ding swap 0-1")
            X0, X1 = X1, X0
            x0, x1 = x1, x0
            a02, a12 = a12, a02
            X01 = _neg(X01)
            X02 = X12
        else:
            br.add("ding no swap (a01 <= a02)")
    a12d = _div(1.0, a12)
    a, b = a01 * a12d, a02 * a12d
    m01, m02, m12 = _dot(x0, x1), _dot(x0, x2), _dot(x1, x2)
    m12sq = -m12 * m12 + 1.0
    m02sq = -1.0 + m02 * m02
    m01sq = -1.0 + m01 * m01
    ab, bsq, asq = a * b, b * b, a * a
    m013 = -2.0 + 2.0 * m01 * m02 * m12
    bsqm12sq, asqm12sq, abm12sq = bsq * m12sq, asq * m12sq, 2.0 * ab * m12sq
    k3_inv = _div(1.0, bsqm12sq + b * m02sq)
    k2 = k3_inv * ((-1.0 + a) * m02sq + abm12sq + bsqm12sq + b * m013)
    k1 = k3_inv * (asqm12sq + abm12sq + a * m013 + (-1.0 + b) * m01sq)
    k0 = k3_inv * (asqm12sq + a * m01sq)
    if not all(math.isfinite(v) for v in (k2, k1, k0)):
        return []
    G, s = _cubic_single_real(k2, k1, k0, mg, br)
    if not math.isfinite(s):
        return []
    C00, C01, C02 = -a + s * (1 - b), -m02 * s, a * m12 + b * m12 * s
    C11, C12, C22 = s + 1, -m01, -a - b * s + 1
    A00, A11, A22 = C12 * C12 - C11 * C22, C02 * C02 - C00 * C22, C01 * C01 - C00 * C11
    A01, A02, A12 = C01 * C22 - C02 * C12, C02 * C11 - C01 * C12, C00 * C12 - C02 * C01
    mg.gap(A00, A11, "pq pivot A00 > A11")
    if A00 > A11:
        mg.gap(A00, A22, "pq pivot A00 > A22")
        col, d = ((A00, A01, A02), A00) if A00 > A22 else ((A02, A12, A22), A22)
    else:
        mg.gap(A11, A22, "pq pivot A11 > A22")
        col, d = ((A01, A11, A12), A11) if A11 > A22 else ((A02, A12, A22), A22)
    q = _sqrt(d)
    v = (_div(col[0], q), _div(col[1], q), _div(col[2], q))
    lines = ((C00, C01 + v[2], C02 - v[1]), (C00, C01 - v[2], C02 + v[1]))
    frame = _frame(X01, X02)
    out = []
    for p0, p1, p2 in lines:
        if not (math.isfinite(p1) and math.isfinite(p2)):
            continue
        switch_12 = abs(p0) <= abs(p1)
        mg.gap(abs(p0), abs(p1), "ding switch_12")
        br.add("ding switch_12" if switch_12 else "ding no switch_12")
        if switch_12:
            w0, w1 = _div(-p0, p1), _div(-p2, p1)
            ca = _div(1.0, w1 * w1 - b)
            cb = 2.0 * (b * m12 - m02 * w1 + w0 * w1) * ca
            cc = (w0 * w0 - 2 * m02 * w0 - b + 1.0) * ca
        else:
            w0, w1 = _div(-p1, p0), _div(-p2, p0)
            ca = _div(1.0, -a * w1 * w1 + 2 * a * m12 * w1 - a + 1)
            cb = 2 * (a * m12 * w0 - m01 - a * w0 * w1) * ca
            cc = (1 - a * w0 * w0) * ca
        ok, t0, t1 = root2real(cb, cc, mg, br)
        if ok:
            for tau in (t0, t1):
                mg.gap(tau, 0.0, "ding tau <= 0", scale=max(abs(t0), abs(t1)))
                if not tau > 0:
                    continue
                if switch_12:
                    d2 = _sqrt(_div(a12, tau * (tau - 2.0 * m12) + 1.0))
                    d1 = tau * d2
                    d0 = (w0 * d2 + w1 * d1)
                    mg.gap(w0 * d2, -(w1 * d1), "ding d0 < 0")
                    if d0 < 0 or d0 != d0:
                        continue
                else:
                    d0 = _sqrt(_div(a01, tau * (tau - 2.0 * m01) + 1.0))
                    d1 = tau * d0
                    d2 = w0 * d0 + w1 * d1
                    mg.gap(w0 * d0, -(w1 * d1), "ding d2 < 0")
                    if d2 < 0 or d2 != d2:
                        continue
                d0, d1, d2 = _ding_refine(d0, d1, d2, a01, a02, a12, m01, m02, m12, mg)
                base = _scale(x0, d0)
                out.append(_pose(frame, X0, _sub(base, _scale(x1, d1)), _sub(base, _scale(x2, d2)), base))
        if out and G:
            break
    return out


def _nordberg_refine(L, a12, a13, a23, b12, b13, b23, mg):
    L1, L2, L3 = L
    for _ in range(5):
        l1, l2, l3 = L1, L2, L3
        r1 = l1 * l1 + l2 * l2 + b12 * l1 * l2 - a12
        r2 = l1 * l1 + l3 * l3 + b13 * l1 * l3 - a13
        r3 = l2 * l2 + l3 * l3 + b23 * l2 * l3 - a23
        s = abs(r1) + abs(r2) + abs(r3)
        mg.gap(s, 1e-10, "nordberg refine stop", scale=1e-10)
        if s < 1e-10:
            break
        v0, v1 = 2.0 * l1 + b12 * l2, 2.0 * l2 + b12 * l1
        v3, v5 = 2.0 * l1 + b13 * l3, 2.0 * l3 + b13 * l1
        v7, v8 = 2.0 * l2 + b23 * l3, 2.0 * l3 + b23 * l2
        det = _div(1.0, -v0 * v5 * v7 - v1 * v3 * v8)
        n1 = l1 - det * (-v5 * v7 * r1 + -v1 * v8 * r2 + v1 * v5 * r3)
        n2 = l2 - det * (-v3 * v8 * r1 + v0 * v8 * r2 + -v0 * v5 * r3)
        n3 = l3 - det * (v3 * v7 * r1 + -v0 * v7 * r2 + -v1 * v3 * r3)
        r11 = n1 * n1 + n2 * n2 + b12 * n1 * n2 - a12
        r12 = n1 * n1 + n3 * n3 + b13 * n1 * n3 - a13
        r13 = n2 * n2 + n3 * n3 + b23 * n2 * n3 - a23
        s1 = abs(r11) + abs(r12) + abs(r13)
        if s1 > s:   # (a residual that grows at the noise floor: either way the depths agree to rounding; not a decision of the loop)
            break
        L1, L2, L3 = n1, n2, n3
    return L1, L2, L3


def _cubick(b, c, d, mg, br):
    mg.gap(b * b, 3.0 * c, "cubick monotonic")
    if b * b >= 3.0 * c:
        v = math.sqrt(b * b - 3.0 * c)
        t1 = (-b - v) / (3.0)
        k = ((t1 + b) * t1 + c) * t1 + d
        mg.gap(k, 0.0, "cubick h(t1) > 0", scale=abs(d) + abs(c * t1) + abs(t1 ** 3))
        if k > 0.0:
            br.add("cubick h(t1) > 0")
            r0 = t1 - _sqrt(_div(-k, 3.0 * t1 + b))
        else:
            br.add("cubick h(t1) <= 0")
            t2 = (-b + v) / 3.0
            k = ((t2 + b) * t2 + c) * t2 + d
            r0 = t2 + _sqrt(_div(-k, 3.0 * t2 + b))
    else:
        br.add("cubick monotonic")
        r0 = -b / 3.0
        if abs(((3.0 * r0 + 2.0 * b) * r0 + c)) < 1e-4:
            r0 += 1
    for cnt in range(50):
        fx = (((r0 + b) * r0 + c) * r0 + d)
        if cnt < 7 or abs(fx) > 1e-13:
            fpx = ((3.0 * r0 + 2.0 * b) * r0 + c)
            r0 -= _div(fx, fpx)
        else:
            break
    return r0


def p3p_nordberg(bear, X, mg=None, br=None):
    mg = Margin() if mg is None else mg
    br = set() if br is None else br
    P1, P2, P3 = (tuple(float(v) for v in X[i]) for i in range(3))
    f1, f2, f3 = (tuple(float(v) for v in bear[i]) for i in range(3))
    b12, b13, b23 = -2.0 * (_dot(f1, f2)), -2.0 * (_dot(f1, f3)), -2.0 * (_dot(f2, f3))
    d12, d13, d23 = _sub(P1, P2), _sub(P1, P3), _sub(P2, P3)
    a12, a13, a23 = _dot(d12, d12), _dot(d13, d13), _dot(d23, d23)
    c31, c23, c12 = -0.5 * b13, -0.5 * b23, -0.5 * b12
    blob = (c12 * c23 * c31 - 1.0)
    s31_squared, s23_squared, s12_squared = 1.0 - c31 * c31, 1.0 - c23 * c23, 1.0 - c12 * c12
    p3 = a13 * (a23 * s31_squared - a13 * s23_squared)
    p2 = 2.0 * blob * a23 * a13 + a13 * (2.0 * a12 + a13) * s23_squared + a23 * (a23 - a12) * s31_squared
    p1 = a23 * (a13 - a23) * s12_squared - a12 * a12 * s23_squared - 2.0 * a12 * (blob * a23 + a13 * s23_squared)
    p0 = a12 * (a12 * s23_squared - a23 * s12_squared)
    p3 = _div(1.0, p3)
    p2 *= p3
    p1 *= p3
    p0 *= p3
    if not all(math.isfinite(v) for v in (p2, p1, p0)):
        return []
    g = _cubick(p2, p1, p0, mg, br)
    if not math.isfinite(g):
        return []
    A00, A01, A02 = a23 * (1.0 - g), (a23 * b12) * 0.5, (a23 * b13 * g) * (-0.5)
    A11, A12, A22 = a23 - a12 + a13 * g, b23 * (a13 * g - a12) * 0.5, g * (a13 - a23) - a12
    x01_squared = A01 * A01
    qb = -A00 - A11 - A22
    qc = -x01_squared - A02 * A02 - A12 * A12 + A00 * (A11 + A22) + A11 * A22
    _, e1, e2 = root2real(qb, qc, mg, br)
    mg.gap(abs(e1), abs(e2), "eigwithknown0 |e1| < |e2|")
    if abs(e1) < abs(e2):
        e1, e2 = e2, e1
    mx0011 = -A00 * A11
    prec_0, prec_1 = A01 * A12 - A02 * A11, A01 * A02 - A00 * A12
    tmp = _div(1.0, e1 * (A00 + A11) + mx0011 - e1 * e1 + x01_squared)
    a1, a2 = -(e1 * A02 + prec_0) * tmp, -(e1 * A12 + prec_1) * tmp
    rnorm = _div(1.0, _sqrt(a1 * a1 + a2 * a2 + 1.0))
    a1 *= rnorm
    a2 *= rnorm
    tmp2 = _div(1.0, e2 * (A00 + A11) + mx0011 - e2 * e2 + x01_squared)
    a21, a22 = -(e2 * A02 + prec_0) * tmp2, -(e2 * A12 + prec_1) * tmp2
    rnorm2 = _div(1.0, _sqrt(a21 * a21 + a22 * a22 + 1.0))
    a21 *= rnorm2
    a22 *= rnorm2
    q = _div(-e2, e1)
    v = math.sqrt(q) if 0.0 < q else 0.0
    frame = _frame(d12, d13)
    out = []
    for s in (v, -v):
        u1, u2, u3 = a1 - s * a21, a2 - s * a22, rnorm - s * rnorm2
        if not all(math.isfinite(u) for u in (u1, u2, u3)):
            continue
        mg.gap(abs(u1), abs(u2), "nordberg |u1| < |u2|")
        triples = []
        if abs(u1) < abs(u2):
            br.add("nordberg |u1| < |u2|")
            a = (a23 - a12) * u3 * u3 - a12 * u2 * u2 + a12 * b23 * u2 * u3
            b = _div(2. * a23 * u1 * u3 - 2. * a12 * u1 * u3 + a12 * b23 * u1 * u2 - a23 * b12 * u2 * u3, a)
            c = _div(a23 * u1 * u1 - a12 * u1 * u1 + a23 * u2 * u2 - a23 * b12 * u1 * u2, a)
            ok, t0, t1 = root2real(b, c, mg, br)
            if not ok:
                continue
            for tau in (t0, t1):
                mg.gap(tau, 0.0, "nordberg tau <= 0", scale=max(abs(t0), abs(t1)))
                if not tau > 0:
                    continue
                l1 = _sqrt(_div(a13, tau * (tau + b13) + 1.))
                l3 = tau * l1
                l2 = _div(-(u1 * l1 + u3 * l3), u2)
                mg.gap(u1 * l1, -(u3 * l3), "nordberg l2 <= 0")
                if not l2 > 0.:
                    continue
                triples.append((l1, l2, l3))
        else:
            br.add("nordberg |u1| >= |u2|")
            w2 = _div(1., -u1)
            w0, w1 = u2 * w2, u3 * w2
            a = _div(1.0, (a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12)
            b = (a13 * b12 * w1 - a12 * b13 * w0 - 2. * w0 * w1 * (a12 - a13)) * a
            c = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a
            ok, t0, t1 = root2real(b, c, mg, br)
            if not ok:
                continue
            for tau in (t0, t1):
                mg.gap(tau, 0.0, "nordberg tau <= 0", scale=max(abs(t0), abs(t1)))
                if not tau > 0.:
                    continue
                d = _div(a23, tau * (b23 + tau) + 1.0)
                l2 = _sqrt(d)
                l3 = tau * l2
                l1 = w0 * l2 + w1 * l3
                mg.gap(w0 * l2, -(w1 * l3), "nordberg l1 <= 0")
                if not l1 > 0.:
                    continue
                triples.append((l1, l2, l3))
        for L in triples:
            l1, l2, l3 = _nordberg_refine(L, a12, a13, a23, b12, b13, b23, mg)
            ry1, ry2, ry3 = _scale(f1, l1), _scale(f2, l2), _scale(f3, l3)
            out.append(_pose(frame, P1, _sub(ry1, ry2), _sub(ry1, ry3), ry1))
    return out


SOLVERS = {DING: p3p_ding, NORDBERG: p3p_nordberg, "ding": p3p_ding, "nordberg": p3p_nordberg}
SOLVERS_BY_NAME = {"ding": DING, "nordberg": NORDBERG}


# ---- the adaptor ----
def bearings(model, intr, x2d):
    return np.array([tri.bearing(model, intr, xy, False) for xy in x2d]).reshape(-1, 3)


def n1_of(model, intr):
    """imagePlane_toCameraPlaneError(1)"""
    return 1.0 / max(float(intr[0]), float(intr[1])) if model == SPHERICAL else 1.0 / float(intr[0])


def residuals(model, intr, P, x2d, X3d):
    """|| (x - project(R X + t, ignore_distortion)) N1 ||^2 of every correspondence; non-finite values as +inf"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        p = X3d @ P[:, :3].T + P[:, 3]
        if model == SPHERICAL:
            w, h = float(intr[0]), float(intr[1])
            k = max(w, h) / (2.0 * math.pi)
            rho = np.sqrt(p[:, 0] * p[:, 0] + p[:, 2] * p[:, 2])
            r0 = np.arctan2(p[:, 0], p[:, 2]) * k + w / 2.0 - x2d[:, 0]
            r1 = -np.arctan2(-p[:, 1], rho) * k + h / 2.0 - x2d[:, 1]
        else:
            iz = 1.0 / p[:, 2]
            u, v = p[:, 0] * iz, p[:, 1] * iz
            f = float(intr[0])
            r0 = float(intr[1]) + u * f - x2d[:, 0]
            r1 = float(intr[2]) + v * f - x2d[:, 1]
        n1 = n1_of(model, intr)
        rx, ry = r0 * n1, r1 * n1
        e = rx * rx + ry * ry
    e[~np.isfinite(e)] = np.inf
    return e


# ---- the exhaustive NFA ----
def logc_tables(n):
    """(logc_n, logc_k) of makelogcombi(3, n): float32 running sums on the table of float log10 values"""
    with np.errstate(divide="ignore"):
        l10 = np.array([math.log10(float(np.float32(i))) if i else -math.inf for i in range(n + 2)], np.float64).astype(np.float32)

    def logcombi(k, m):
        if k >= m:
            return np.float32(0.0)
        if m - k < k:
            k = m - k
        i = np.arange(1, k + 1)
        return np.cumsum(l10[m - i + 1] - l10[i], dtype=np.float32)[-1] if k else np.float32(0.0)
    # logc_n: the running sum over i shared by all k (k' = min(k, n - k) terms)
    i = np.arange(1, n // 2 + 1)
    run = np.cumsum(l10[n - i + 1] - l10[i], dtype=np.float32) if n >= 2 else np.zeros(0, np.float32)
    logc_n = np.zeros(n + 1, np.float32)
    for k in range(1, n):
        logc_n[k] = run[min(k, n - k) - 1]
    logc_k = np.array([logcombi(3, m) for m in range(n + 1)], np.float32)
    return logc_n, logc_k


def nfa_scan(e, loge0, logc_n, logc_k):
    """(order, nfa over k = 4..n): order = the indices by (residual, index) ascending"""
    n = len(e)
    order = np.lexsort((np.arange(n), e))
    r = e[order]
    k = np.arange(4, n + 1)
    with np.errstate(all="ignore"):
        logalpha = LOGALPHA0 + np.log10(r[3:] + FLT_EPS)
        nfa = ((loge0 + logalpha * (k - 3).astype(np.float64)) + logc_n[4:].astype(np.float64)) + logc_k[4:].astype(np.float64)
    return order, r, nfa


# ---- KRt_From_P ----
def krt_from_p(P):
    P = np.asarray(P, np.float64).reshape(3, 4)
    K = P[:, :3].copy()
    Q = np.eye(3)
    if K[2, 1] != 0:
        c, s = -K[2, 2], K[2, 1]
        l = math.hypot(c, s)
        c, s = c / l, s / l
        Qx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
        K, Q = K @ Qx, Qx.T @ Q
    if K[2, 0] != 0:
        c, s = K[2, 2], K[2, 0]
        l = math.hypot(c, s)
        c, s = c / l, s / l
        Qy = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        K, Q = K @ Qy, Qy.T @ Q
    if K[1, 0] != 0:
        c, s = -K[1, 1], K[1, 0]
        l = math.hypot(c, s)
        c, s = c / l, s / l
        Qz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        K, Q = K @ Qz, Qz.T @ Q
    R = Q
    if K[2, 2] < 0:
        K, R = -K, -R
    if K[1, 1] < 0:
        S = np.diag([1.0, -1.0, 1.0])
        K, R = K @ S, S @ R
    if K[0, 0] < 0:
        S = np.diag([-1.0, 1.0, 1.0])
        K, R = K @ S, S @ R
    t = np.linalg.solve(K, P[:, 3])
    if np.linalg.det(R) < 0:
        R, t = -R, -t
    return K / K[2, 2], R, t


# ---- the loop ----
class Run:
    """ok, R, t, C, P, error_max (pixels), min_nfa, inliers (ascending residual), n_iterations, n_models, margin, margin_where,
    trace: [(iteration, what)] with what in "better", "pool" (vec_index = vec_inliers), "extend" (++nIter; --nIterReserve),
    undecided_at: the first iteration whose sample holds a point whose place in the pool is rounding noise (None: the run is decided)"""


def localize(model, intr, x2d, X3d, solver=DING, max_iteration=4096, heads=None):
    """heads: {iteration: head of the sorted list of the iteration's winning model} as ANOTHER implementation ran it (the device's
    trace). Where a list's members with noise-level residuals (UNORDERED_BELOW_PX) are the same set there, they take that order - the one
    thing two correct runs may differ in - so that this run draws the same samples; undecided_at then stays None."""
    x2d = np.asarray(x2d, np.float64).reshape(-1, 2)
    X3d = np.asarray(X3d, np.float64).reshape(-1, 3)
    n = len(x2d)
    out = Run()
    out.ok, out.R, out.t, out.C, out.P = False, None, None, None, None
    out.error_max, out.min_nfa, out.inliers = 0.0, 0.0, np.zeros(0, np.uint32)
    out.n_iterations = out.n_models = 0
    out.margin, out.margin_where, out.trace, out.branches, out.undecided_at, out.unordered = math.inf, None, [], set(), None, set()
    if n <= 3:
        return out
    solve = SOLVERS[solver]
    mg = Margin()
    bear = bearings(model, intr, x2d)
    logc_n, logc_k = logc_tables(n)
    loge0 = math.log10(4.0 * (n - 3))
    bg = tri._mt19937()
    pool = list(range(n))
    min_nfa, error_max = math.inf, math.inf
    inliers, best_P, inliers_unordered = [], None, set()
    out.undecided_at = None
    reserve = max_iteration // 10
    n_iter = max_iteration - reserve
    it = 0
    n1 = n1_of(model, intr)
    unordered = set()   # members of the adopted pool whose mutual order is rounding noise (see UNORDERED_BELOW_PX)
    while it < n_iter and it < max_iteration:
        last = len(pool) - 1
        for i in range(3):
            s = i + tri._below(bg, last - i + 1)
            pool[i], pool[s] = pool[s], pool[i]
        sample = pool[:3]
        if out.undecided_at is None and unordered.intersection(sample):
            out.undecided_at = it
        better = False
        for M in solve(bear[sample], X3d[sample], mg, out.branches):
            if not np.all(np.isfinite(M)):
                continue   # the one deliberate difference: the reference would sort NaNs
            out.n_models += 1
            order, r, nfa = nfa_scan(residuals(model, intr, M, x2d, X3d), loge0, logc_n, logc_k)
            j = int(np.argmin(nfa))   # the first minimum: the lowest k
            best = float(nfa[j])
            if math.isfinite(min_nfa):
                mg.gap(best, min_nfa, f"nfa < minNFA (iteration {it})")
            if best < min_nfa:
                k = j + 4
                better = True
                min_nfa, error_max, best_P = best, float(r[k - 1]), M
                inliers = [int(v) for v in order[:k]]
                noise = [int(v) for v, e in zip(order[:k], r[:k]) if math.sqrt(e) / n1 < UNORDERED_BELOW_PX]
                inliers_unordered = set(noise) if len(noise) > 1 else set()
                out.trace.append((it, "better"))
                if len(nfa) > 1:
                    second = float(np.partition(nfa, 1)[1])
                    mg.gap(best, second, f"winning k against its runner-up (iteration {it})")
                for a, b in ((k - 2, k - 1), (k - 1, k)):
                    if 0 <= a and b < n and math.isfinite(r[b]) and r[a] != r[b]:   # (equal to the bit: a tie, decided by the index)
                        mg.gap(float(r[a]), float(r[b]), f"sorted residuals next to k (iteration {it})")
                mg.gap(min_nfa, 0.0, f"minNFA < 0 (iteration {it})", scale=1.0)
        if better and heads is not None and inliers_unordered:
            theirs = [v for v in heads.get(it, ()) if v in inliers_unordered]
            if set(theirs) == inliers_unordered:   # (else: left as it is, and the comparison of the runs fails)
                order_of = iter(theirs)
                inliers = [next(order_of) if v in inliers_unordered else v for v in inliers]
                inliers_unordered = set()
        if (better and min_nfa < 0) or ((it + 1) == n_iter and reserve > 0):
            if not inliers:
                n_iter += 1
                reserve -= 1
                out.trace.append((it, "extend"))
            else:
                pool = list(inliers)
                unordered = inliers_unordered
                out.trace.append((it, "pool"))
                if reserve:
                    n_iter = it + 1 + reserve
                    reserve = 0
        it += 1
    out.n_iterations = it
    out.unordered = set(inliers_unordered)   # members of the returned list whose mutual order is rounding noise
    out.min_nfa = min_nfa
    out.margin, out.margin_where = mg.value, mg.where
    if min_nfa >= 0:
        inliers = []
    out.inliers = np.array(inliers, np.uint32)
    out.error_max = math.sqrt(error_max) / n1_of(model, intr) if inliers else error_max
    if len(inliers) > 2.5 * 3:
        out.ok = True
        out.P = np.array(best_P)
        _, out.R, out.t = krt_from_p(best_P)
        out.C = -out.R.T @ out.t
    return out


# ---- inputs ----
def intrinsics_of(model, rng):
    intr = np.zeros(8)
    if model == SPHERICAL:
        intr[:2] = (2000.0, 1000.0)
    else:
        intr[:3] = (1000.0 + 200.0 * rng.random(), 640.0 + 10.0 * rng.random(), 480.0 + 10.0 * rng.random())
        if model == RADIAL3:
            intr[3:6] = (-0.1, 0.02, -0.003)   # must be ignored: the pixels come with the distortion removed
    return intr


def project(model, intr, p):
    """the undistorted pixel of camera-frame points"""
    if model == SPHERICAL:
        w, h = intr[0], intr[1]
        k = max(w, h) / (2.0 * math.pi)
        rho = np.sqrt(p[:, 0] ** 2 + p[:, 2] ** 2)
        return np.stack([np.arctan2(p[:, 0], p[:, 2]) * k + w / 2.0, -np.arctan2(-p[:, 1], rho) * k + h / 2.0], 1)
    return np.stack([intr[1] + intr[0] * p[:, 0] / p[:, 2], intr[2] + intr[0] * p[:, 1] / p[:, 2]], 1)


def problem(n, model=PINHOLE, outliers=0.3, noise=0.5, seed=0):
    """n correspondences of one view: points in a box in front of a random pose, pixels with gaussian noise, a share of them replaced by
    uniform positions. Returns dict(model, intr, x2d, X3d, R, t, is_outlier)."""
    rng = np.random.default_rng(seed)
    intr = intrinsics_of(model, rng)
    R = np.array(tri.rotation(rng.normal(size=3) * 0.3))
    t = rng.normal(size=3) * 0.5 + (0.0, 0.0, 6.0)
    pc = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 3.0, n)], 1)   # camera frame, z = 4 .. 9 after the shift
    pc[:, 2] += 6.0
    X = (pc - t) @ R   # R^T (p - t)
    x = project(model, intr, X @ R.T + t) + rng.normal(size=(n, 2)) * noise
    is_out = np.zeros(n, bool)
    is_out[rng.permutation(n)[: int(round(outliers * n))]] = True
    w, h = (intr[0], intr[1]) if model == SPHERICAL else (2.0 * intr[1], 2.0 * intr[2])
    x[is_out] = np.stack([rng.uniform(0, w, is_out.sum()), rng.uniform(0, h, is_out.sum())], 1)
    return dict(model=model, intr=intr, x2d=np.ascontiguousarray(x), X3d=np.ascontiguousarray(X), R=R, t=t, is_outlier=is_out)


def p3p_samples(n, seed=0):
    """n noise-free samples: (bearings (n, 3, 3), X (n, 3, 3), R (n, 3, 3), t (n, 3))"""
    rng = np.random.default_rng(seed)
    B, Xs, Rs, ts = [], [], [], []
    for _ in range(n):
        R = np.array(tri.rotation(rng.normal(size=3) * 0.6))
        t = rng.normal(size=3) + (0.0, 0.0, 5.0)
        pc = np.stack([rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3), rng.uniform(2, 9, 3)], 1)
        B.append(pc / np.linalg.norm(pc, axis=1, keepdims=True))
        Xs.append((pc - t) @ R)
        Rs.append(R)
        ts.append(t)
    return np.array(B), np.array(Xs), np.array(Rs), np.array(ts)
