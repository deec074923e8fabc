"""What the emulation and the GPU accuracy tests of mvgx_triangulate_tracks share: the families of tests/golden/triangulation_truth.npz
(hard geometry: scenes away from the origin, small parallax), one call of the library per family and solver, and the limit

    E_dev <= max(10 x E_ref, 1000 x SPREAD[solver])

with E_dev = max |X_device - X*|, E_ref = max |X_restatement - X*| read from the fixture (never from the code under test) and X* the
50-digit point of tests/_triangulation_truth.py. The factor 10 over the reference's own error: E_ref is the maximum of a heavy-tailed
sample (10 - 100 x its median), and two backward-stable solvers of one problem differ by modest constants. The second term is the
rule of tests/_triangulation_cases.py for benign inputs."""
import functools
import importlib.util
import os

import numpy as np

from tests import _triangulation_cases as cases
from tests import _triangulation_ref as ref
from tests import _triangulation_truth as truth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 10.0
SPREAD_OF = {"dlt": "dlt", "l1": "closed", "linf": "closed", "midpoint": "closed", "nview": "nview"}
FAMILIES = range(5)


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_triangulation_truth", os.path.join(GOLDEN, "make_triangulation_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "triangulation_truth.npz")) as z:
        return {k: z[k] for k in z.files}


# (name, views, solver, keywords of the call): every call triangulates ALL observations of every track
CALLS = [("blind", 3, "nview", dict(mode="blind")), ("blind", 4, "nview", dict(mode="blind")), ("blind", 12, "nview", dict(mode="blind")),
         ("robust-3-3", 3, "nview", dict(mode="robust", min_required_inliers=3, min_sample_index=3)),
         ("blind", 2, "midpoint", dict(mode="blind"))]
CALLS += [("robust-2-2", 2, s, dict(mode="robust", method=truth.METHOD_OF[s], min_required_inliers=2, min_sample_index=2))
          for s in ("dlt", "l1", "linf", "midpoint")]
CALL_IDS = [f"{name}-{views}-{solver}" for name, views, solver, _ in CALLS]


def family_scene(family, views):
    """the tracks of one scene of the fixture as the arrays of mvgx_triangulate_tracks: every track has poses of its own"""
    fx = fixture()
    poses, xy = fx[f"f{family}_v{views}_poses"], fx[f"f{family}_v{views}_xy"]
    n = len(poses)
    intr = np.zeros((1, 8))
    intr[0, :3] = fx["intr"]
    return dict(poses=poses.reshape(-1, 6), intrinsics=intr, intr_model=np.array([ref.PINHOLE], np.int32),
                track_start=(views * np.arange(n + 1)).astype(np.uint64), obs_pose=np.arange(n * views, dtype=np.uint32),
                obs_intr=np.zeros(n * views, np.uint32), obs_xy=xy.reshape(-1, 2))


def limit(family, views, solver):
    """(E_ref, the limit on E_dev) from the fixture"""
    fx = fixture()
    key = f"f{family}_v{views}_{solver}_"
    e_ref = float(truth.error(fx[key + "ref"], fx[key + "hi"], fx[key + "lo"]).max())
    return e_ref, max(FACTOR * e_ref, 1000.0 * cases.SPREAD[SPREAD_OF[solver]])


def check(family, name, views, solver, kw):
    fx = fixture()
    key = f"f{family}_v{views}_{solver}_"
    X, ok, inl, _ = cases.run_device(family_scene(family, views), **kw)
    e_ref, bound = limit(family, views, solver)
    e_dev = float(truth.error(X, fx[key + "hi"], fx[key + "lo"]).max())
    offset, baseline = fx["families"][family]
    print(f"offset {offset:g} baseline {baseline:g} | {name} {views} views {solver}: E_dev {e_dev:.3g}, E_ref {e_ref:.3g}, ratio {e_dev / e_ref:.3g}, "
          f"limit {bound:.3g}")
    assert ok.all() and inl.all(), "a track whose 50-digit decisions all have margin was rejected"
    assert e_dev <= bound, (e_dev, e_ref, e_dev / e_ref)
    return e_dev, e_ref
