"""Writes tests/golden/resection_bounded_golden.npz: the REFERENCE's ACRANSAC with a finite `precision` (quantified NFA, max-consensus
warm-up, early exit; robust_estimator_ACRansac.hpp) over the reference's Ding solver, on the 108 runs of the bounded parity grid:
PARITY_MODELS x outliers 0 / 0.3 / 0.6 x max_iteration 9 / 10 / 40 / 4096 x error_max 1 / 4 / 16 px (tests/_resection_bounded_cases.py).
Per run: inlier list, threshold, minNFA, model and the residual vector of the winning model; and the spreads between the float64
restatement (tests/_resection_bounded_ref.py) and the compiled reference, which set the device tests' tolerances and margin guard.

Run by hand on the machine that has the reference tree (REFERENCE_SRC, default /root/reference/src). Like make_resection_golden.py it
compiles a driver of our own text - that file's loop driver with the precision read per run and the winning model's residuals written out -
against the tree into a temporary directory and keeps nothing compiled.
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_resection_golden as mk  # noqa: E402
from tests import _resection_bounded_ref as bref  # noqa: E402
from tests import _resection_ref as ref  # noqa: E402

GOLD_PATH = os.path.join(ROOT, "tests", "golden", "resection_bounded_golden.npz")


def _edit(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


# the exhaustive loop driver with three changes: a precision (squared pixels, what SfM_Localizer::Localize passes: Square(error_max)) per
# run, handed to ACRANSAC; and after the run the residuals of the returned model under the driver's own Errors
DRIVER = mk.LOOP_DRIVER
DRIVER = _edit(DRIVER, "fread(&A.n1, sizeof(double), 1, in) != 1) return 1;",
               "fread(&A.n1, sizeof(double), 1, in) != 1) return 1;\n    double precision = 0.0;\n    if (fread(&precision, sizeof(double), 1, in) != 1) return 1;")
DRIVER = _edit(DRIVER, "&P, std::numeric_limits<double>::infinity(), false);", "&P, precision, false);")
DRIVER = _edit(DRIVER, "if (k) fwrite(inliers.data(), sizeof(uint32_t), k, out);",
               "if (k) fwrite(inliers.data(), sizeof(uint32_t), k, out);\n    std::vector<double> e;\n    A.Errors(P, e);\n    fwrite(e.data(), sizeof(double), e.size(), out);")


def run_reference(runs):
    """runs: [(problem dict, max_iteration, error_max px)] -> [(inliers, error_max, min_nfa, P, residuals of P)]"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = mk.compile_driver(tmp, DRIVER, "bounded_loop_driver")
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.int32(len(runs)).tobytes())
            for pr, it, em in runs:
                n = len(pr["x2d"])
                f.write(np.array([n, pr["model"], it], np.int32).tobytes() + np.asarray(pr["intr"], np.float64).tobytes() +
                        np.float64(ref.n1_of(pr["model"], pr["intr"])).tobytes() + np.float64(em * em).tobytes() +
                        np.ascontiguousarray(pr["x2d"]).tobytes() + np.ascontiguousarray(pr["X3d"]).tobytes() +
                        np.ascontiguousarray(ref.bearings(pr["model"], pr["intr"], pr["x2d"])).tobytes())
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, at = [], 0
    for pr, _, _ in runs:
        n = len(pr["x2d"])
        k, = struct.unpack_from("i", raw, at)
        err, nfa = struct.unpack_from("2d", raw, at + 4)
        P = np.frombuffer(raw, np.float64, 12, at + 20).reshape(3, 4).copy()
        inl = np.frombuffer(raw, np.uint32, k, at + 116).copy()
        e = np.frombuffer(raw, np.float64, n, at + 116 + 4 * k).copy()
        at += 116 + 4 * k + 8 * n
        out.append((inl, err, nfa, P, e))
    assert at == len(raw)
    return out


if __name__ == "__main__":
    from tests import _resection_bounded_cases as cases  # noqa: E402
    grid = cases.PARITY_GRID
    problems = {(m, o): cases.parity_problem(m, o) for m, o, _, _ in grid}
    got = run_reference([(problems[(m, o)], it, em) for m, o, it, em in grid])
    same_list, nfa_bits, thr_bits = [], [], []
    P_spread = e_spread = nfa_diff = thr_diff = 0.0
    margins = []
    for (m, o, it, em), (inl, err, nfa, P, e) in zip(grid, got):
        pr = problems[(m, o)]
        own = bref.localize_bounded(m, pr["intr"], pr["x2d"], pr["X3d"], em, max_iteration=it)
        margins.append(own.margin)
        same = np.array_equal(inl, own.inliers)
        same_list.append(same)
        nfa_bits.append(nfa == own.min_nfa)
        thr_bits.append(err == own.error_max)
        if not nfa_bits[-1] and np.isfinite(nfa):
            nfa_diff = max(nfa_diff, abs(nfa - own.min_nfa) / max(abs(nfa), 1.0))
        if not thr_bits[-1] and np.isfinite(err):
            thr_diff = max(thr_diff, abs(err - own.error_max) / abs(err))
        if same and len(inl):
            P_spread = max(P_spread, float(np.abs(P - own.model).max()))
            # relative to what a residual is compared with: the nearest bin edge is at least maxThreshold / 20, and at least the residual's size
            fin = np.isfinite(e) & np.isfinite(own.residuals)
            scale = np.maximum(np.abs(e[fin]), own.max_threshold / bref.N_BINS)
            e_spread = max(e_spread, float(np.max(np.abs(e[fin] - own.residuals[fin]) / scale)))
    arrays = dict(grid=np.array(grid, np.float64), same_list=np.array(same_list), nfa_bits=np.array(nfa_bits), thr_bits=np.array(thr_bits),
                  min_nfa=np.array([r[2] for r in got]), error_max=np.array([r[1] for r in got]), P=np.array([r[3] for r in got]),
                  n_inliers=np.array([len(r[0]) for r in got]), inliers=np.concatenate([r[0] for r in got]).astype(np.uint32),
                  n_residuals=np.array([len(r[4]) for r in got]), residuals=np.concatenate([r[4] for r in got]),
                  own_margin=np.array(margins), spread=np.array([P_spread, e_spread, nfa_diff, thr_diff]))
    np.savez_compressed(GOLD_PATH, **arrays)
    print("runs", len(grid), "with a model", int(np.sum(arrays["n_inliers"] > 0)), "| restatement returns the reference's list in", int(np.sum(same_list)),
          "| minNFA equal to the bit in", int(np.sum(nfa_bits)), "threshold in", int(np.sum(thr_bits)))
    print("spreads: |dP|", P_spread, "relative residual", e_spread, "minNFA", nfa_diff, "threshold", thr_diff)
    print("restatement's margins: smallest", min(margins), "| below 1000 x residual spread:", int(np.sum(np.array(margins) < 1000.0 * e_spread)),
          "|", os.path.getsize(GOLD_PATH), "bytes")
