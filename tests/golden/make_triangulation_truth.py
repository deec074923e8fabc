"""Writes tests/golden/triangulation_truth.npz: pinhole tracks on hard geometry (scenes away from the origin, small parallax), the
50-digit point of every solver on them (tests/_triangulation_truth.py) as a float64 pair, the float64 restatement's point
(tests/_triangulation_ref.py) and, where oracle/_ref/libref_geofilter.so is built, the compiled reference's Triangulate2View.

  python tests/golden/make_triangulation_truth.py [tracks per family, default 100]

Five families (offset of the scene from the origin, camera baseline), each with scenes of 2, 3, 4 and 12 views; every track has cameras
of its own: a grid of centres `baseline` apart at depth 5 in front of the point, rotations of sigma 0.05 rad away from the common
viewing direction, pixel noise of sigma 0.5. Offset 1e5 with a baseline of 0.05 is deliberately absent: there the float64 reference
itself collapses. Every track comes from a seed of its own (family, views, candidate index), so any of them can be made again alone:
tests/test_triangulation_accuracy_emu_cpu.py regenerates ten per scene and compares."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _triangulation_ref as ref  # noqa: E402
from tests import _triangulation_truth as truth  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "triangulation_truth.npz")
FAMILIES = ((0.0, 1.0), (0.0, 0.05), (1e3, 1.0), (1e3, 0.05), (1e5, 1.0))   # (offset, baseline)
VIEWS = (2, 3, 4, 12)
SOLVERS_OF = {2: ("dlt", "l1", "linf", "midpoint"), 3: ("nview",), 4: ("nview",), 12: ("nview",)}
INTR = (1000.0, 500.0, 500.0)
DEPTH, NOISE, ROTATION_SIGMA, MAX_REPROJECTION_ERROR = 5.0, 0.5, 0.05, 4.0
# Where the scene lies, seen from the origin: along the world's x axis, across the viewing direction. Along a general direction the
# float64 N-view reference collapses at offset 1e5 (errors of 0.1 .. 4 at depth 5 for (0.6, -0.48, 0.64), (0.8, -0.6, 0) and the
# diagonal, seen while this was written): no yardstick, and the second condition of scene() refuses such a family.
DIRECTION = np.array([1.0, 0.0, 0.0])
SEED = 20261020
# conditions on the INPUTS (against the 50-digit point): every track is kept by every correct solver, whatever its rounding
MAX_R2 = 0.5 * MAX_REPROJECTION_ERROR ** 2
MIN_DOT = 0.1
MIN_BRANCH_MARGIN = 1e-6
MAX_LEFT_OUT = 0.05
MAX_RESTATEMENT_ERROR = 1e-2 * DEPTH


def track(family, views, index):
    """candidate `index` of a scene -> poses (views, 6), xy (views, 2)"""
    from scipy.spatial.transform import Rotation
    offset, baseline = FAMILIES[family]
    rng = np.random.default_rng([SEED, family, views, index])
    origin = offset * DIRECTION
    X = origin + rng.uniform(-0.5, 0.5, 3)
    cols = min(views, 4)
    rows = (views + cols - 1) // cols
    poses, xy = np.zeros((views, 6)), np.zeros((views, 2))
    for i in range(views):
        grid = np.array([i % cols - (cols - 1) / 2, i // cols - (rows - 1) / 2, 0.0])
        C = origin + baseline * (grid + np.array([0.2, 0.2, 0.1]) * rng.standard_normal(3)) - np.array([0.0, 0.0, DEPTH])
        aa = ROTATION_SIGMA * rng.standard_normal(3)
        R = Rotation.from_rotvec(aa).as_matrix()
        t = -R @ C
        p = R @ X + t
        poses[i, :3], poses[i, 3:] = aa, t
        xy[i] = (INTR[1] + INTR[0] * p[0] / p[2], INTR[2] + INTR[0] * p[1] / p[2]) + NOISE * rng.standard_normal(2)
    return poses, xy


def usable(t):
    return t["ok"] and max(t["r2"]) < MAX_R2 and min(t["dot"]) > MIN_DOT and all(m > MIN_BRANCH_MARGIN for m in t["margins"])


def restatement(solver, poses, xy):
    """the float64 restatement on one track -> (ok, X)"""
    intr = list(INTR) + [0.0] * 5
    cams = [(ref.rotation(p[:3]), tuple(float(v) for v in p[3:6]), ref.bearing(ref.PINHOLE, intr, x, True)) for p, x in zip(poses, xy)]
    if solver == "nview":
        return True, ref.nview_algebraic([ref.nview_cost(*c) for c in cams])
    return ref.two_view(truth.METHOD_OF[solver], *cams[0], *cams[1])


def compiled_reference(fn, solver, poses, xy):
    intr = list(INTR) + [0.0] * 5
    cams = [(ref.rotation(p[:3]), tuple(float(v) for v in p[3:6]), ref.bearing(ref.PINHOLE, intr, x, True)) for p, x in zip(poses, xy)]
    return fn(truth.METHOD_OF[solver], *cams[0], *cams[1])


def one(family, views, index, fn=None):
    """candidate -> None if it misses the input conditions, else dict(poses, xy, solver -> dict(hi, lo, ref[, cref]))"""
    poses, xy = track(family, views, index)
    out = dict(poses=poses, xy=xy)
    for solver in SOLVERS_OF[views]:
        t = truth.solve(solver, poses, INTR, xy)
        if not usable(t):
            return None
        ok, X = restatement(solver, poses, xy)
        assert ok, "the float64 restatement rejects a track the 50-digit solver keeps with margin"
        out[solver] = dict(hi=np.array(t["hi"]), lo=np.array(t["lo"]), ref=np.array(X))
        if fn is not None and views == 2:
            ok, X = compiled_reference(fn, solver, poses, xy)
            assert ok
            out[solver]["cref"] = np.array(X)
    return out


def scene(family, views, n_tracks, fn=None):
    """-> (dict of arrays keyed as in the file, left out)"""
    kept, index = [], []
    i = 0
    while len(kept) < n_tracks:
        got = one(family, views, i, fn)
        if got is not None:
            kept.append(got); index.append(i)
        i += 1
        assert i <= 2 * n_tracks + 20, f"family {family}, {views} views: most tracks miss the input conditions"
    if n_tracks >= 50:
        assert i - len(kept) <= MAX_LEFT_OUT * i, f"family {family}, {views} views: {i - len(kept)} of {i} tracks miss the input conditions"
    key = f"f{family}_v{views}_"
    arrays = {key + "index": np.array(index, np.int32), key + "poses": np.stack([k["poses"] for k in kept]), key + "xy": np.stack([k["xy"] for k in kept])}
    for solver in SOLVERS_OF[views]:
        for field in kept[0][solver]:
            arrays[key + solver + "_" + field] = np.stack([k[solver][field] for k in kept])
        e_ref = truth.error(arrays[key + solver + "_ref"], arrays[key + solver + "_hi"], arrays[key + solver + "_lo"]).max()
        print(f"family {FAMILIES[family]}, {views} views, {solver}: {len(kept)} tracks, {i - len(kept)} left out, restatement vs 50 digits {e_ref:.3g}",
              flush=True)
        assert e_ref <= MAX_RESTATEMENT_ERROR, "the float64 reference is no yardstick on this family"
    return arrays, i - len(kept)


def main():
    n_tracks = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    fn = None
    from tests import test_triangulation_ref_cpu as compiled
    if os.path.exists(compiled.REF_SO):
        fn = compiled.compiled_two_view()
    arrays = dict(intr=np.array(INTR), families=np.array(FAMILIES), n_tracks=np.array(n_tracks))
    for family in range(len(FAMILIES)):
        left = 0
        for views in VIEWS:
            a, n = scene(family, views, n_tracks, fn)
            arrays.update(a); left += n
        print(f"family {FAMILIES[family]}: {left} tracks left out in all")
    np.savez_compressed(PATH, **arrays)
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
