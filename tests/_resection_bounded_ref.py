"""Float64 restatement of the reference's robust resection with a BOUNDED precision - the yardstick of the bounded resection tests
(TEST INFRASTRUCTURE). On top of tests/_resection_ref.py (solvers, residuals, logcombi tables, generator, KRt_From_P) it restates
  robust_estimation/robust_estimator_ACRansac.hpp:205-256   the NFA read off a 20-bin histogram of the residuals
  third_party/histogram/histogram.hpp:49-61, :74-86, :105-112   bin index, and the bin VALUES (max / 19 b), which are not the bins' edges
  robust_estimation/robust_estimator_ACRansac.hpp:351-358, :375, :383-475   maxThreshold, the max-consensus warm-up, the early exit
  robust_estimation/rand_sampling.hpp:36-58   UniformSample(3, nData, ...): a repeated index is drawn again
The NFA of a bin is a fixed-order sum of host doubles and float table entries - no transcendental per model - so minNFA and the threshold
are equal to the bit between two implementations whenever the counts agree.

A run's DECISION MARGIN is the smallest relative distance of any evaluated residual to what it is compared with: a bin edge 1..20 of the
histogram (the lower edge of bin 0 is no edge), maxThreshold in the warm-up, the chosen bin value when a list is built - and the solvers'
own branch margins. Exact NFA ties are ties (the earlier model / lower bin wins in every implementation), not margin 0.

Deliberate differences from the reference, shared with the device: a model with a non-finite entry is skipped; an adopted pool of fewer
than three entries stops the run with its current result.
"""
import math

import numpy as np

from tests import _resection_ref as ref
from tests import _triangulation_ref as tri

N_BINS = 20


def bound_constants(model, intr, error_max):
    """(maxThreshold, nBins_by_interval, bin values, logalpha per bin value) as the reference forms them"""
    n1 = ref.n1_of(model, intr)
    max_threshold = error_max * error_max * n1 * n1   # Square(error_max) * N(0,0) * N(0,0)
    nbi = N_BINS / (max_threshold - 0.0)
    val = (max_threshold - 0.0) / float(N_BINS - 1)
    bin_value = [val * float(b) + 0.0 for b in range(N_BINS)]
    logalpha = [ref.LOGALPHA0 + 1.0 * math.log10(v + ref.FLT_EPS) for v in bin_value]
    return max_threshold, nbi, bin_value, logalpha


def histogram_nfa(e, nbi, bin_value, logalpha, loge0, logc_n, logc_k):
    """(best NFA or inf, its bin value, the cumulated counts): the first bin of strictly smallest NFA among the negative ones"""
    with np.errstate(all="ignore"):
        t = e * nbi
    inside = t < N_BINS   # (a non-finite residual lands in no bin)
    hist = np.bincount(t[inside].astype(np.int64), minlength=N_BINS)
    best, thr, cum = math.inf, 0.0, 0
    cums = []
    for b in range(N_BINS):
        cum += int(hist[b])
        cums.append(cum)
        if cum > 3 and bin_value[b] > ref.FLT_EPS:
            nfa = ((loge0 + logalpha[b] * float(cum - 3)) + float(logc_n[cum])) + float(logc_k[cum])
            if nfa < best and nfa < 0:
                best, thr = nfa, bin_value[b]
    return best, thr, cums


def edge_margin(e, nbi):
    """smallest relative distance of a residual to a bin edge 1..20"""
    with np.errstate(all="ignore"):
        t = e[np.isfinite(e)] * nbi
    if not len(t):
        return math.inf
    k = np.clip(np.rint(t), 1, N_BINS)
    return float(np.min(np.abs(t - k) / k))


def value_margin(e, v):
    f = e[np.isfinite(e)]
    return float(np.min(np.abs(f - v) / v)) if len(f) and v > 0 else math.inf


def localize_bounded(model, intr, x2d, X3d, error_max, solver=ref.DING, max_iteration=4096):
    """Run (tests/_resection_ref.py) of the bounded loop; inliers in ascending index order. Besides: switch_at (the iteration that turned
    the a-contrario mode on, None: never), n_nfa (NFA values produced), short_lists (lists rebuilt that failed the size test),
    residuals (of the winning model), stopped (the pool rule)."""
    x2d = np.asarray(x2d, np.float64).reshape(-1, 2)
    X3d = np.asarray(X3d, np.float64).reshape(-1, 3)
    n = len(x2d)
    out = ref.Run()
    out.ok, out.R, out.t, out.C, out.P = False, None, None, None, None
    out.error_max, out.min_nfa, out.inliers = 0.0, 0.0, np.zeros(0, np.uint32)
    out.n_iterations = out.n_models = 0
    out.margin, out.margin_where, out.trace, out.branches = math.inf, None, [], set()
    out.switch_at, out.n_nfa, out.short_lists, out.residuals, out.stopped = None, 0, 0, None, False
    if n <= 3:
        return out
    solve = ref.SOLVERS[solver]
    mg = ref.Margin()
    bear = ref.bearings(model, intr, x2d)
    logc_n, logc_k = ref.logc_tables(n)
    loge0 = math.log10(4.0 * (n - 3))
    max_threshold, nbi, bin_value, logalpha = bound_constants(model, intr, error_max)
    bg = tri._mt19937()
    pool = list(range(n))
    min_nfa, threshold = math.inf, math.inf
    inliers, best_P, best_e = [], None, None
    reserve = max_iteration // 10
    n_iter = max_iteration - reserve
    it = 0
    ac = False
    n1 = ref.n1_of(model, intr)

    def note(value, where):
        if value < mg.value:
            mg.value, mg.where = value, where

    while it < n_iter and it < max_iteration:
        if ac:
            last = len(pool) - 1
            for i in range(3):
                s = i + tri._below(bg, last - i + 1)
                pool[i], pool[s] = pool[s], pool[i]
            sample = pool[:3]
        else:
            sample = []
            while len(sample) < 3:
                s = tri._below(bg, n)
                if s not in sample:
                    sample.append(s)
        better = False
        for M in solve(bear[sample], X3d[sample], mg, out.branches):
            if not np.all(np.isfinite(M)):
                continue
            out.n_models += 1
            e = ref.residuals(model, intr, M, x2d, X3d)
            if not ac:
                note(value_margin(e, max_threshold), f"maxThreshold in the warm-up (iteration {it})")
                if int(np.sum(e <= max_threshold)) > 2.5 * 3:
                    ac = True
                    out.switch_at = it
                    out.trace.append((it, "switch"))
            if ac:
                note(edge_margin(e, nbi), f"bin edge (iteration {it})")
                best, thr, cums = histogram_nfa(e, nbi, bin_value, logalpha, loge0, logc_n, logc_k)
                out.n_nfa += sum(1 for b in range(N_BINS) if cums[b] > 3 and bin_value[b] > ref.FLT_EPS)
                if best < min_nfa:
                    note(value_margin(e, thr), f"chosen bin value (iteration {it})")
                    inliers = [int(i) for i in np.flatnonzero(e <= thr)]   # rebuilt before its size decides
                    if len(inliers) > 3:
                        better = True
                        min_nfa, threshold, best_P, best_e = best, thr, M, e
                        out.trace.append((it, "better"))
                    else:
                        out.short_lists += 1
        if not ac and it > reserve * 2:
            out.trace.append((it, "early exit"))
            it += 1
            break
        if ac and ((better and min_nfa < 0) or ((it + 1) == n_iter and reserve > 0)):
            if not inliers:
                n_iter += 1
                reserve -= 1
                out.trace.append((it, "extend"))
            else:
                pool = list(inliers)
                out.trace.append((it, "pool"))
                if reserve:
                    n_iter = it + 1 + reserve
                    reserve = 0
                if len(pool) < 3:
                    out.stopped = True
                    it += 1
                    break
        it += 1
    out.n_iterations = it
    out.min_nfa = min_nfa
    out.margin, out.margin_where = mg.value, mg.where
    if min_nfa >= 0:
        inliers = []
    out.inliers = np.array(inliers, np.uint32)
    out.error_max = math.sqrt(threshold) / n1 if inliers else threshold
    out.threshold = threshold   # normalised, squared: a bin value
    out.max_threshold = max_threshold
    out.residuals = best_e
    if best_P is not None:
        out.model = np.array(best_P)
    if len(inliers) > 2.5 * 3:
        out.ok = True
        out.P = np.array(best_P)
        _, out.R, out.t = ref.krt_from_p(best_P)
        out.C = -out.R.T @ out.t
    return out
