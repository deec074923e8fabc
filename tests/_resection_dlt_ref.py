"""Float64 restatement of the reference's resection of a view WITHOUT intrinsics - the yardstick of the uncalibrated resection tests
(TEST INFRASTRUCTURE).

What is restated (paths under src/openMVG of the reference):
  sfm/pipelines/localization/SfM_Localizer.cpp:134-161, :321-331             the DLT_6POINTS branch of SfM_Localizer::Localize
  robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:203-288     ACKernelAdaptorResection, UnnormalizerResection
  multiview/conditioning.cpp:54-77                                           NormalizePoints by the image size
  multiview/solver_resection_kernel.cpp:29-136                               SixPointResectionSolver::Solve (np.linalg.svd for the null space)
  multiview/solver_resection_metrics.hpp:28-39                               SquaredPixelReprojectionError
  robust_estimation/robust_estimator_ACRansac.hpp:257-304, :326-489          the exhaustive NFA, the a-contrario loop
  robust_estimation/rand_sampling.hpp:71-100                                 UniformSample on the pool (six swaps)
KRt_From_P, the generator with its bounded draw, the logcombi(k, n) table, Margin and the problems come from tests/_resection_ref.py and
tests/_triangulation_ref.py.

Decision margins (tests/_resection_ref.py) are taken, besides the loop's, on the solver's two gates: the ratio of the second smallest to
the largest singular value against 1e-5 (relative distance) and the cheirality test (smallest |depth| of the six over the largest)."""
import math

import numpy as np

from tests import _resection_ref as ref
from tests import _triangulation_ref as tri

SAMPLE = 6
RATIO_GATE = 1e-5
IMAGE_WH = (1280, 960)


def normalizer(w, h):
    """(dNorm, offset x, offset y) of PreconditionerFromPoints(width, height): the x offset through a float product (-.5f * width)"""
    d = 1.0 / math.sqrt(float(int(w) * int(h)))
    return d, float(np.float32(-0.5) * np.float32(int(w))) * d, -0.5 * int(h) * d


def normalize(x2d, w, h):
    d, ox, oy = normalizer(w, h)
    x2d = np.asarray(x2d, np.float64).reshape(-1, 2)
    return np.stack([d * x2d[:, 0] + ox, d * x2d[:, 1] + oy], 1)


def unnormalize(P, w, h):
    """N1^-1 P, the inverse by back substitution of the identity (Eigen's PartialPivLU of the upper triangular N1)"""
    d, ox, oy = normalizer(w, h)
    i00, i02, i12 = 1.0 / d, (0.0 - ox) / d, (0.0 - oy) / d
    P = np.asarray(P, np.float64).reshape(3, 4)
    return np.stack([i00 * P[0] + i02 * P[2], i00 * P[1] + i12 * P[2], P[2]])


def _givens_signs(P):
    """the diagonal of K after the three Givens steps of KRt_From_P, before the sign fixes (for the record of branches alone)"""
    K = np.asarray(P, np.float64).reshape(3, 4)[:, :3].copy()
    for (a, b), (ci, si), sign in (((2, 1), (2, 2), -1.0), ((2, 0), (2, 2), 1.0), ((1, 0), (1, 1), -1.0)):
        if K[a, b] != 0:
            c, s = sign * K[ci, si], K[a, b]
            l = math.hypot(c, s)
            c, s = c / l, s / l
            if (a, b) == (2, 1):
                Q = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
            elif (a, b) == (2, 0):
                Q = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
            else:
                Q = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
            K = K @ Q
    return K[0, 0], K[1, 1], K[2, 2]


def design_matrix(xn, X):
    X = np.asarray(X, np.float64).reshape(SAMPLE, 3)
    Xt = X - X[0]
    A = np.zeros((12, 12))
    for i in range(SAMPLE):
        h = [float(Xt[i, 0]), float(Xt[i, 1]), float(Xt[i, 2]), 1.0]
        for c in range(2):
            x = float(xn[i][c])
            row = [0.0] * 12
            for e in range(4):
                row[4 * c + e] = h[e]
                row[8 + e] = -x * h[e]
            n2 = 0.0
            for v in row:
                n2 += v * v
            A[2 * i + c] = np.array(row) / math.sqrt(n2) if n2 > 0.0 else row
    return A


def six_point(xn, X, mg=None, br=None):
    """SixPointResectionSolver::Solve(x, X, &Ps, bcheck = true) on six normalised pixels: ([P] or [], ratio)"""
    xn = np.asarray(xn, np.float64).reshape(SAMPLE, 2)
    X = np.asarray(X, np.float64).reshape(SAMPLE, 3)
    A = design_matrix(xn, X)
    if not np.all(np.isfinite(A)):
        return [], math.nan
    _, S, Vt = np.linalg.svd(A)
    ratio = float(S[10] / S[0]) if S[0] > 0 else math.nan
    if mg is not None and math.isfinite(ratio):
        mg.gap(ratio, RATIO_GATE, "ratio gate")
    if not ratio > RATIO_GATE:
        if br is not None:
            br.add("ratio rejected")
        return [], ratio
    P = Vt[11].reshape(3, 4).copy()
    t = -X[0]
    P[:, 3] = ((P[:, 0] * t[0] + P[:, 1] * t[1]) + P[:, 2] * t[2]) + P[:, 3]
    with np.errstate(all="ignore"):
        P = P / P[2, 3]
    if not np.all(np.isfinite(P)):
        return [P], ratio   # (the loop skips it)
    K, R, tt = ref.krt_from_p(P)
    depth = (R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1]) + R[2, 2] * X[:, 2] + tt[2]
    if mg is not None:
        mg.gap(float(np.abs(depth).min()), 0.0, "cheirality", scale=float(np.abs(depth).max()))
    if br is not None:
        k00, k11, k22 = _givens_signs(P)
        if k22 < 0:
            br.add("K(2,2) < 0")
        if (k11 < 0) != (k22 < 0):
            br.add("K(1,1) < 0")
        if (k00 < 0) != (k22 < 0):
            br.add("K(0,0) < 0")
        flips = int(k22 < 0) + int((k11 < 0) != (k22 < 0)) + int((k00 < 0) != (k22 < 0))   # the Givens product has det +1; every fix flips it
        if flips % 2:
            br.add("det R < 0")
        br.add("in front" if np.all(depth > 0) else "depth rejected")
    if not np.all(depth > 0):
        return [], ratio
    return [P], ratio


def residuals(P, xn, X3d):
    """| x - hnormalized(P (X, 1)) |^2 in normalised pixels, the sums in the reference's order; non-finite values as +inf"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    X, Y, Z = X3d[:, 0], X3d[:, 1], X3d[:, 2]
    with np.errstate(all="ignore"):
        u = ((P[0, 0] * X + P[0, 1] * Y) + P[0, 2] * Z) + P[0, 3]
        v = ((P[1, 0] * X + P[1, 1] * Y) + P[1, 2] * Z) + P[1, 3]
        w = ((P[2, 0] * X + P[2, 1] * Y) + P[2, 2] * Z) + P[2, 3]
        rx, ry = xn[:, 0] - u / w, xn[:, 1] - v / w
        e = rx * rx + ry * ry
    e[~np.isfinite(e)] = np.inf
    return e


def logc_tables(n):
    """(logc_n, logc_k) of makelogcombi(6, n): float32 running sums on the table of float log10 values"""
    logc_n, _ = ref.logc_tables(n)
    with np.errstate(divide="ignore"):
        l10 = np.array([math.log10(float(np.float32(i))) if i else -math.inf for i in range(n + 2)], np.float64).astype(np.float32)
    logc_k = np.zeros(n + 1, np.float32)
    for m in range(n + 1):
        k = SAMPLE
        if k >= m:
            continue
        if m - k < k:
            k = m - k
        i = np.arange(1, k + 1)
        logc_k[m] = np.cumsum(l10[m - i + 1] - l10[i], dtype=np.float32)[-1] if k else np.float32(0.0)
    return logc_n, logc_k


def nfa_scan(e, loge0, logc_n, logc_k):
    """(order, sorted residuals, nfa over k = 7..n): order = the indices by (residual, index) ascending"""
    n = len(e)
    order = np.lexsort((np.arange(n), e))
    r = e[order]
    k = np.arange(SAMPLE + 1, n + 1)
    with np.errstate(all="ignore"):
        logalpha = ref.LOGALPHA0 + np.log10(r[SAMPLE:] + ref.FLT_EPS)
        nfa = ((loge0 + logalpha * (k - SAMPLE).astype(np.float64)) + logc_n[SAMPLE + 1:].astype(np.float64)) + logc_k[SAMPLE + 1:].astype(np.float64)
    return order, r, nfa


def localize(x2d, X3d, image_wh=IMAGE_WH, max_iteration=4096, heads=None):
    """The Run of tests/_resection_ref.py, with K: P is the unnormalised projection matrix, K, R, t = KRt_From_P(P). heads: as
    _resection_ref.localize's (the order of noise-level residuals as another implementation ran it). Besides: min_ratio_decades (the
    nearest a sample came to the ratio gate, in decades) and n_ratio_rejected."""
    x2d = np.asarray(x2d, np.float64).reshape(-1, 2)
    X3d = np.asarray(X3d, np.float64).reshape(-1, 3)
    n = len(x2d)
    w, h = int(image_wh[0]), int(image_wh[1])
    out = ref.Run()
    out.ok, out.R, out.t, out.C, out.P, out.K = False, None, None, None, None, None
    out.error_max, out.min_nfa, out.inliers = 0.0, 0.0, np.zeros(0, np.uint32)
    out.n_iterations = out.n_models = 0
    out.margin, out.margin_where, out.trace, out.branches, out.undecided_at, out.unordered = math.inf, None, [], set(), None, set()
    out.min_ratio_decades = math.inf
    if n <= SAMPLE:
        return out
    mg = ref.Margin()
    d_norm = normalizer(w, h)[0]
    xn = normalize(x2d, w, h)
    logc_n, logc_k = logc_tables(n)
    loge0 = math.log10(float(n - SAMPLE))
    bg = tri._mt19937()
    pool = list(range(n))
    min_nfa, error_max = math.inf, math.inf
    inliers, best_P, inliers_unordered = [], None, set()
    reserve = max_iteration // 10
    n_iter = max_iteration - reserve
    it = 0
    unordered = set()
    while it < n_iter and it < max_iteration:
        last = len(pool) - 1
        for i in range(SAMPLE):
            s = i + tri._below(bg, last - i + 1)
            pool[i], pool[s] = pool[s], pool[i]
        sample = pool[:SAMPLE]
        if out.undecided_at is None and unordered.intersection(sample):
            out.undecided_at = it
        better = False
        models, ratio = six_point(xn[sample], X3d[sample], mg, out.branches)
        if math.isfinite(ratio) and ratio > 0:
            out.min_ratio_decades = min(out.min_ratio_decades, abs(math.log10(ratio / RATIO_GATE)))
        for M in models:
            if not np.all(np.isfinite(M)):
                continue   # a deliberate difference: the reference would sort NaNs
            out.n_models += 1
            order, r, nfa = nfa_scan(residuals(M, xn, X3d), loge0, logc_n, logc_k)
            j = int(np.argmin(nfa))   # the first minimum: the lowest k
            best = float(nfa[j])
            if math.isfinite(min_nfa):
                mg.gap(best, min_nfa, f"nfa < minNFA (iteration {it})")
            if best < min_nfa:
                k = j + SAMPLE + 1
                better = True
                min_nfa, error_max, best_P = best, float(r[k - 1]), M
                inliers = [int(v) for v in order[:k]]
                noise = [int(v) for v, e in zip(order[:k], r[:k]) if math.sqrt(e) / d_norm < ref.UNORDERED_BELOW_PX]
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
            if set(theirs) == inliers_unordered:
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
    out.unordered = set(inliers_unordered)
    out.min_nfa = min_nfa
    out.margin, out.margin_where = mg.value, mg.where
    if min_nfa >= 0:
        inliers = []
    out.inliers = np.array(inliers, np.uint32)
    out.error_max = math.sqrt(error_max) / d_norm if inliers else error_max
    if len(inliers) > 2.5 * SAMPLE:
        out.ok = True
        out.P = unnormalize(best_P, w, h)
        out.K, out.R, out.t = ref.krt_from_p(out.P)
        out.C = -out.R.T @ out.t
    return out


def intrinsic_seed(K):
    """sequential_SfM.cpp:986-987"""
    return (K[0, 0] + K[1, 1]) / 2.0, float(K[0, 2]), float(K[1, 2])


# ---- inputs ----
def parity_problem(outliers, s):
    """the parity grid's problems: pinhole views of 60 + 7 int(10 o) + s correspondences, 0.5 px noise"""
    return ref.problem(60 + 7 * int(10 * outliers) + s, ref.PINHOLE, outliers, noise=0.5, seed=100 * s + int(10 * outliers))


def _view(rng):
    R = np.array(tri.rotation(rng.normal(size=3) * 0.5))
    t = rng.normal(size=3) * 0.5 + (0.0, 0.0, 6.0)
    f, cx, cy = 1000.0 + 200.0 * rng.random(), 640.0 + 10.0 * rng.random(), 480.0 + 10.0 * rng.random()
    return R, t, f, cx, cy


def solver_samples(n=400, seed=0, noise=0.5):
    """(x_norm (m, 6, 2), X (m, 6, 3), group (m)): n general six-point samples with `noise` px of gaussian noise (group 0); then the three
    depth outcomes - all six in front (1), one behind the camera (2), all behind (3), 12 each, mirrored image axes among them -; then
    near-coplanar sextuples whose thickness sweeps the ratio gate (4)"""
    rng = np.random.default_rng(seed)
    xs, Xs, groups = [], [], []

    def add(pc, view, group, flip=(1.0, 1.0)):
        R, t, f, cx, cy = view
        X = (pc - t) @ R
        x = np.stack([cx + flip[0] * f * pc[:, 0] / pc[:, 2], cy + flip[1] * f * pc[:, 1] / pc[:, 2]], 1) + rng.normal(size=(SAMPLE, 2)) * noise
        xs.append(normalize(x, *IMAGE_WH))
        Xs.append(X)
        groups.append(group)

    def box():
        return np.stack([rng.uniform(-2.5, 2.5, SAMPLE), rng.uniform(-2.0, 2.0, SAMPLE), rng.uniform(4.0, 9.0, SAMPLE)], 1)

    for _ in range(n):
        add(box(), _view(rng), 0)
    for i in range(12):
        flip = ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))[i % 4]   # a mirrored axis: K's sign fixes and det R < 0
        add(box(), _view(rng), 1, flip)
        pc = box()
        pc[3] *= -1.0   # one point behind the camera: its pixel is the point reflection's
        add(pc, _view(rng), 2, flip)
        add(-box(), _view(rng), 3, flip)
    for thickness in np.logspace(-7.0, -1.0, 25):   # points within `thickness` of a plane: the second smallest singular value follows it
        pc = box()
        pc[:, 2] = 6.0 + 0.2 * pc[:, 0] - 0.1 * pc[:, 1] + thickness * rng.normal(size=SAMPLE)
        add(pc, _view(rng), 4)
    return np.array(xs), np.array(Xs), np.array(groups)
