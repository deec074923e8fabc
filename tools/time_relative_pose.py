"""Times the relative pose of image pairs on the MI355X: mvgx_relative_pose_from_essential (the cheirality stage alone) and
mvgx_relative_pose_robust (robustRelativePose from start to end) at the two caller settings of the reference.

  python tools/time_relative_pose.py [--pairs 1000] [--sizes 200,2000] [--repeat 5] [--outliers 0.3]

Prints one JSON line per (entry, pair size): kernel_ms = HIP events around the cheirality kernel (mvgx_relative_pose_stats.kernel_ms),
acransac_kernel_ms = those around the a-contrario stage before it, total_ms = the whole call with uploads, downloads and the host's
packing; medians over --repeat calls after one warm-up call. stage_share = kernel_ms / (kernel_ms + acransac_kernel_ms): the share of the
robust call's device time that the new stage takes. Needs a GPU: there is no CPU path.
The reference's time for the same work is that of the driver of tests/golden/make_relative_pose_golden.py on one CPU thread (see
DESIGN.md, "Relative pose")."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openmvg_amd import _capi, geofilter   # noqa: E402
from openmvg_amd import relative_pose as rp   # noqa: E402

WH, FOCAL = (1000, 1000), 1000.0
K = np.array([[FOCAL, 0.0, 500.0], [0.0, FOCAL, 500.0], [0.0, 0.0, 1.0]])


def make_pairs(n_pairs, n, outliers, seed=0xE2):
    """pairs of pinhole views of points 2 .. 8 deep: a rotation of 0.1 .. 0.4 rad, a unit baseline, 0.5 px noise, a share of uniform outliers"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((n_pairs, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    R = Rotation.from_rotvec(axis * rng.uniform(0.1, 0.4, (n_pairs, 1))).as_matrix()
    t = rng.uniform(0.3, 1.0, (n_pairs, 3)) * rng.choice([-1.0, 1.0], (n_pairs, 3)); t /= np.linalg.norm(t, axis=1, keepdims=True)
    X = np.stack([rng.uniform(-2, 2, (n_pairs, n)), rng.uniform(-2, 2, (n_pairs, n)), rng.uniform(2, 8, (n_pairs, n))], axis=2)
    Y = np.einsum("pij,pnj->pni", R, X) + t[:, None]
    xI = X[..., :2] / X[..., 2:] * FOCAL + 500.0 + 0.5 * rng.standard_normal((n_pairs, n, 2))
    xJ = Y[..., :2] / Y[..., 2:] * FOCAL + 500.0 + 0.5 * rng.standard_normal((n_pairs, n, 2))
    bad = rng.random((n_pairs, n)) < outliers
    xJ[bad] = rng.uniform(0.0, 1000.0, (int(bad.sum()), 2))
    E = np.einsum("pij,pjk->pik", np.stack([np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]) for v in t]), R)
    start = (np.arange(n_pairs + 1) * n).astype(np.uint64)
    return xI.reshape(-1, 2), xJ.reshape(-1, 2), start, E


def median_of(calls, repeat):
    calls()   # warm-up: code objects, the slab caches
    rows = [calls() for _ in range(repeat)]
    return {k: float(np.median([getattr(st, k) for st in rows])) for k in ("kernel_ms", "acransac_kernel_ms", "total_ms")}, rows[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--sizes", default="200,2000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--outliers", type=float, default=0.3)
    a = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("time_relative_pose.py needs a GPU")
    for n in (int(v) for v in a.sizes.split(",")):
        xI, xJ, start, E = make_pairs(a.pairs, n, a.outliers)
        wh = np.tile(np.array(WH * 2, np.uint32), (a.pairs, 1))
        Ks = np.tile(K.reshape(1, 1, 3, 3), (a.pairs, 2, 1, 1))
        bI, bJ = geofilter.pinhole_bearings(K, xI), geofilter.pinhole_bearings(K, xJ)
        med, st = median_of(lambda: rp.from_essential_raw(E, bI, bJ, start)[4], a.repeat)
        print(json.dumps(dict(entry="from_essential", pairs=a.pairs, correspondences=n, **med, pairs_ok=int(st.n_pairs_ok), selected=int(st.n_selected))), flush=True)
        for tolerance, iterations in ((2.5 * 2.5, 256), (4.0 * 4.0, 4096)):
            med, st = median_of(lambda: rp.robust(xI, xJ, start, wh, Ks, tolerance, iterations, bearings=(bI, bJ))[2], a.repeat)
            share = med["kernel_ms"] / max(med["kernel_ms"] + med["acransac_kernel_ms"], 1e-12)
            print(json.dumps(dict(entry="robust", pairs=a.pairs, correspondences=n, tolerance=tolerance, iterations=iterations, **med, stage_share=share,
                                  pairs_ok=int(st.n_pairs_ok), selected=int(st.n_selected))), flush=True)


if __name__ == "__main__":
    main()
