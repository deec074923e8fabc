"""50-digit restatement of the reference's triangulation solvers - the yardstick of the accuracy tests (TEST INFRASTRUCTURE).

Where tests/_triangulation_ref.py restates the reference in float64 (and is itself only good to rounding times the conditioning of the
problem), this module computes what the reference's FORMULATIONS give in exact arithmetic, from the raw inputs of a pinhole track: the
angle-axis rows and translations, f, cx, cy and the pixels, each taken as the exact value of its double.
  R                  Rodrigues, c I + s [w]x + (1 - c) w w^T
  bearing            ((x - cx) / f, (y - cy) / f, 1).normalized()
  "nview"            TriangulateNViewAlgebraic (multiview/triangulation_nview.cpp:39-61): AtA = sum cost^T cost, cost = P - b b^T P, the
                     eigenvector of the smallest eigenvalue, hnormalized
  "dlt"              TriangulateDLT (multiview/triangulation.cpp:16-70): the right singular vector of the smallest singular value of D
  "l1", "linf", "midpoint"   the three closed forms of Triangulate2View (:116-216)
It is the formulation that is restated, not the geometric point: a solver is measured against what it is meant to compute.
Pinhole only - the other models' undistortions are iterative, and the ring-family tests pin them.
"""
from mpmath import mp, mpf

DPS = 50
SOLVERS = ("dlt", "l1", "linf", "midpoint", "nview")
METHOD_OF = {"dlt": 0, "l1": 1, "linf": 2, "midpoint": 3}   # ETriangulationMethod


def _vec(v):
    return [mpf(float(x)) for x in v]


def rotation(aa):
    a0, a1, a2 = _vec(aa)
    th2 = a0 * a0 + a1 * a1 + a2 * a2
    if th2 == 0:
        return [[mpf(1), mpf(0), mpf(0)], [mpf(0), mpf(1), mpf(0)], [mpf(0), mpf(0), mpf(1)]]
    th = mp.sqrt(th2)
    c, s = mp.cos(th), mp.sin(th)
    k = 1 - c
    w0, w1, w2 = a0 / th, a1 / th, a2 / th
    return [[c + k * w0 * w0, -s * w2 + k * w0 * w1, s * w1 + k * w0 * w2],
            [s * w2 + k * w1 * w0, c + k * w1 * w1, -s * w0 + k * w1 * w2],
            [-s * w1 + k * w2 * w0, s * w0 + k * w2 * w1, c + k * w2 * w2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _normalized(a):
    n = mp.sqrt(_dot(a, a))
    return [a[0] / n, a[1] / n, a[2] / n]


def _axpy(s, x, y):
    return [s * x[i] + y[i] for i in range(3)]


def bearing(f, cx, cy, xy):
    return _normalized([(mpf(float(xy[0])) - cx) / f, (mpf(float(xy[1])) - cy) / f, mpf(1)])


def _to_camera(R, t, X):
    return [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]


def _to_world(R, t, x):
    d = [x[i] - t[i] for i in range(3)]
    return [R[0][j] * d[0] + R[1][j] * d[1] + R[2][j] * d[2] for j in range(3)]


def _relative(a, b):
    """relative distance of the two sides of a comparison"""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m != 0 else mpf(0)


def _cosine(a, b):
    n = mp.sqrt(_dot(a, a) * _dot(b, b))
    return abs(_dot(a, b)) / n if n != 0 else mpf(0)


def _nview(cams, bs):
    A = mp.zeros(4)
    for (R, t), b in zip(cams, bs):
        P = mp.matrix([[R[i][0], R[i][1], R[i][2], t[i]] for i in range(3)])
        bv = mp.matrix(b)   # already of unit length
        cost = P - bv * (bv.T * P)
        A += cost.T * cost
    E, Q = mp.eigsy(A)
    c = min(range(4), key=lambda i: E[i])
    return [Q[i, c] / Q[3, c] for i in range(3)]


def _dlt(cams, bs):
    rows = []
    for (R, t), x in zip(cams, bs):
        P = [[R[i][0], R[i][1], R[i][2], t[i]] for i in range(3)]
        rows.append([x[0] * P[2][j] - x[2] * P[0][j] for j in range(4)])
        rows.append([x[1] * P[2][j] - x[2] * P[1][j] for j in range(4)])
    _, S, V = mp.svd_r(mp.matrix(rows))
    r = min(range(4), key=lambda i: S[i])
    X = [V[r, i] / V[r, 3] for i in range(3)]
    depth = [_to_camera(R, t, X)[2] for R, t in cams]
    return all(d > 0 for d in depth), X, [abs(d) / mp.sqrt(_dot(X, X) + 1) for d in depth]


def _point_from_rays(m0, m1, t, R1, t1):
    z = _cross(m1, m0)
    c0, c1 = _cross(t, m1), _cross(t, m0)
    z2 = _dot(z, z)
    l0, l1 = _dot(z, c0) / z2, _dot(z, c1) / z2
    X = _to_world(R1, t1, _axpy(l0, m0, t))
    return (l0 > 0 and l1 > 0), X, [_cosine(z, c0), _cosine(z, c1)]   # l0, l1 > 0: the sign of a dot product, relative to its factors


def _closed(solver, cams, bs):
    (R0, t0), (R1, t1) = cams
    x0, x1 = bs
    R = [[sum(R1[i][k] * R0[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
    t = [t1[i] - _dot(R[i], t0) for i in range(3)]
    Rx0 = [_dot(R[i], x0) for i in range(3)]
    if solver == "l1":
        ca, cb = _cross(_normalized(Rx0), t), _cross(_normalized(x1), t)
        branch = _relative(_dot(ca, ca), _dot(cb, cb))
        if _dot(ca, ca) <= _dot(cb, cb):
            n1 = _normalized(_cross(x1, t))
            ok, X, m = _point_from_rays(_axpy(-_dot(Rx0, n1), n1, Rx0), x1, t, R1, t1)
        else:
            n0 = _normalized(_cross(Rx0, t))
            ok, X, m = _point_from_rays(Rx0, _axpy(-_dot(x1, n0), n0, x1), t, R1, t1)
        return ok, X, [branch] + m
    if solver == "linf":
        rn, xn = _normalized(Rx0), _normalized(x1)
        na = _cross([rn[i] + xn[i] for i in range(3)], t)
        nb = _cross([rn[i] - xn[i] for i in range(3)], t)
        branch = _relative(_dot(na, na), _dot(nb, nb))
        n = _normalized(na) if _dot(na, na) >= _dot(nb, nb) else _normalized(nb)
        ok, X, m = _point_from_rays(_axpy(-_dot(Rx0, n), n, Rx0), _axpy(-_dot(x1, n), n, x1), t, R1, t1)
        return ok, X, [branch] + m
    assert solver == "midpoint"
    cp, cq, cr = _cross(Rx0, x1), _cross(Rx0, t), _cross(x1, t)
    pn, qn, rn = mp.sqrt(_dot(cp, cp)), mp.sqrt(_dot(cq, cq)), mp.sqrt(_dot(cr, cr))
    w, rp, qp = qn / (qn + rn), rn / pn, qn / pn
    X = _to_world(R1, t1, [w * (t[i] + rp * (Rx0[i] + x1[i])) for i in range(3)])
    l0, l1 = [rp * v for v in Rx0], [qp * v for v in x1]

    def sq(s0, s1):
        e = [t[i] + s0 * l0[i] + s1 * l1[i] for i in range(3)]
        return _dot(e, e)
    mm, others = sq(1, -1), min(sq(1, 1), sq(-1, -1), sq(-1, 1))
    return mm < others, X, [_relative(mm, others)]


def solve(solver, poses, intr, xy):
    """One pinhole track: poses (n, 6: angle-axis | t), intr (f, cx, cy), xy (n, 2), all doubles taken exactly. Returns a dict:
    ok (the solver's own verdict), hi / lo (float64 pair of the 50-digit point: X* = hi + lo to 32 digits), margins (relative margin of
    every branch and verdict of the solver, floats), r2 and dot (per observation: residual^2 in px^2 and the cheirality dot product
    bearing . pose(X*), against the 50-digit point)."""
    with mp.workdps(DPS):
        f, cx, cy = _vec(intr[:3])
        cams = [(rotation(p[:3]), _vec(p[3:6])) for p in poses]
        bs = [bearing(f, cx, cy, x) for x in xy]
        if solver == "nview":
            ok, X, margins = True, _nview(cams, bs), []
        elif solver == "dlt":
            ok, X, margins = _dlt(cams, bs)
        else:
            ok, X, margins = _closed(solver, cams, bs)
        r2, dots = [], []
        for (R, t), b, x in zip(cams, bs, xy):
            p = _to_camera(R, t, X)
            dots.append(float(_dot(b, p)))
            u, v = cx + f * p[0] / p[2] - mpf(float(x[0])), cy + f * p[1] / p[2] - mpf(float(x[1]))
            r2.append(float(u * u + v * v))
        hi = [float(v) for v in X]
        lo = [float(v - mpf(h)) for v, h in zip(X, hi)]
        return dict(ok=bool(ok), hi=hi, lo=lo, margins=[float(m) for m in margins], r2=r2, dot=dots)


def error(X, hi, lo):
    """|X - X*| per coordinate for float64 arrays X against the stored pair: (X - hi) - lo, the first difference exact where X is within a
    factor of two of hi (Sterbenz), which is every case in which the error matters."""
    return abs((X - hi) - lo)
