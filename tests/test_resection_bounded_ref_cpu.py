"""CPU: the float64 restatement of the bounded resection loop (tests/_resection_bounded_ref.py) against the compiled reference's ACRANSAC
with a finite precision, recorded in tests/golden/resection_bounded_golden.npz (tests/golden/make_resection_bounded_golden.py) on the 108
runs of the bounded parity grid."""
import numpy as np

from tests import _resection_bounded_cases as cases
from tests import _resection_bounded_ref as bref


def test_fixture_covers_the_grid():
    g = cases.gold()
    assert np.array_equal(g["grid"], np.array(cases.PARITY_GRID, np.float64)) and len(g["grid"]) == 108
    assert int(np.sum(g["n_inliers"] > 0)) == 78   # runs that return a model; every 0.6-outlier run at 9 / 10 / 40 iterations exits early
    for i, (m, o, it, em) in enumerate(cases.PARITY_GRID):
        if o == 0.6 and it < 4096:
            assert g["n_inliers"][i] == 0 and np.isinf(g["min_nfa"][i])
    P_spread, e_spread, nfa_diff, thr_diff = cases.spreads()
    print(f"spreads restatement - compiled reference: |dP| {P_spread:.3g}, relative residual {e_spread:.3g}, minNFA {nfa_diff:.3g}, threshold {thr_diff:.3g}; "
          f"guard {cases.guard():.3g}")
    assert 0.0 < e_spread < 1e-6 and 0.0 < P_spread < 1e-9


def test_restatement_matches_the_compiled_reference():
    """on every run whose decision margin is at least the guard: the inlier list exactly, minNFA and threshold to the bit (or within 1 000 x
    the difference the fixture recorded), the model and its residual vector within 10 x the recorded spreads; at most 5 % left out"""
    P_spread, e_spread, nfa_diff, thr_diff = cases.spreads()
    left_out = []
    smallest = np.inf
    for i, (m, o, it, em) in enumerate(cases.PARITY_GRID):
        pr = cases.parity_problem(m, o)
        own = cases.restated(("parity", m, o), pr, em, it)
        smallest = min(smallest, own.margin)
        if own.margin < cases.guard():
            left_out.append((m, o, it, em, own.margin, own.margin_where))
            continue
        want = cases.gold_run(i)
        assert np.array_equal(own.inliers, want["inliers"]), (m, o, it, em)
        assert cases.close_or_equal(own.min_nfa, want["min_nfa"], nfa_diff), (m, o, it, em, own.min_nfa, want["min_nfa"])
        assert cases.close_or_equal(own.error_max, want["error_max"], thr_diff), (m, o, it, em, own.error_max, want["error_max"])
        if len(want["inliers"]):
            assert np.abs(own.model - want["P"]).max() <= 10.0 * P_spread
            e = want["residuals"]
            fin = np.isfinite(e) & np.isfinite(own.residuals)
            scale = np.maximum(np.abs(e[fin]), own.max_threshold / bref.N_BINS)
            assert np.max(np.abs(e[fin] - own.residuals[fin]) / scale) <= 10.0 * e_spread
    print(f"smallest margin {smallest:.3g}; left out {len(left_out)} of {len(cases.PARITY_GRID)}: {left_out}")
    assert len(left_out) <= 0.05 * len(cases.PARITY_GRID)


def test_bin_values_are_not_bin_edges():
    """histogram.hpp:105-112: value b = max / 19 b, edge b = max / 20 b; the last value is the bound itself"""
    pr = cases.parity_problem(1, 0.0)
    max_threshold, nbi, values, logalpha = bref.bound_constants(pr["model"], pr["intr"], 4.0)
    assert values[0] == 0.0 and values[19] == max_threshold / 19.0 * 19.0 and nbi == 20 / max_threshold
    assert all(values[b] > b / nbi for b in range(1, 20))
