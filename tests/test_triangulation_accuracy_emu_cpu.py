"""CPU: the points of mvgx_triangulate_tracks under the HIP emulation (tests/_emu.py) against 50-digit solutions on hard geometry -
scenes away from the origin and small parallax, where the float64 restatement is no yardstick to rounding any more
(tests/_triangulation_accuracy_cases.py has the rule). The -m gpu twin is tests/test_triangulation_accuracy_gpu.py. Also here: the
fixture against its generator."""
import numpy as np
import pytest

from tests import _emu
from tests import _triangulation_accuracy_cases as acc
from tests import _triangulation_truth as truth


@pytest.fixture()
def emulated():
    with _emu.emulated():
        yield


@pytest.mark.parametrize("family", acc.FAMILIES)
@pytest.mark.parametrize("name,views,solver,kw", acc.CALLS, ids=acc.CALL_IDS)
def test_points_against_50_digits(emulated, family, name, views, solver, kw):
    acc.check(family, name, views, solver, kw)


@pytest.mark.parametrize("family", acc.FAMILIES)
def test_fixture_regenerates(family):
    """ten tracks of every scene, made again from their seeds: inputs and 50-digit pairs bit for bit; the restatement's point to within
    its own error against the truth (LAPACK builds differ in rounding, and on these families rounding is what its error is)"""
    gen, fx = acc.generator(), acc.fixture()
    assert np.array_equal(fx["intr"], gen.INTR) and np.array_equal(fx["families"], gen.FAMILIES)
    for views in gen.VIEWS:
        key = f"f{family}_v{views}_"
        for row in range(10):
            got = gen.one(family, views, int(fx[key + "index"][row]))
            assert got is not None
            assert np.array_equal(got["poses"], fx[key + "poses"][row]) and np.array_equal(got["xy"], fx[key + "xy"][row])
            for solver in gen.SOLVERS_OF[views]:
                hi, lo = fx[key + solver + "_hi"], fx[key + solver + "_lo"]
                assert np.array_equal(got[solver]["hi"], hi[row]) and np.array_equal(got[solver]["lo"], lo[row])
                e_ref = truth.error(fx[key + solver + "_ref"], hi, lo).max()
                assert np.abs(got[solver]["ref"] - fx[key + solver + "_ref"][row]).max() <= e_ref


def test_truth_reproduces_an_exact_point():
    """a scene whose every number is a dyadic rational (identity rotations, the point (0.5, 0.25, 4), pixels on half-pixel positions):
    the rays meet exactly, and every 50-digit solver returns that point to 45 digits; then the pair hi + lo carries more than a double on
    a track of the fixture's families"""
    poses = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, -1.0, 0, 0], [0, 0, 0, 0, -1.0, 0]], np.float64)
    xy = np.array([[625.0, 562.5], [375.0, 562.5], [625.0, 312.5]])
    for solver in ("dlt", "l1", "linf", "midpoint"):
        t = truth.solve(solver, poses[:2], (1000.0, 500.0, 500.0), xy[:2])
        assert t["ok"] and t["hi"] == [0.5, 0.25, 4.0] and max(abs(v) for v in t["lo"]) < 1e-45 and max(t["r2"]) < 1e-80
        assert min(t["dot"]) > 3.9   # (the scene is symmetric: the branch margins of the angular methods are zero here)
    t = truth.solve("nview", poses, (1000.0, 500.0, 500.0), xy)
    assert t["hi"] == [0.5, 0.25, 4.0] and max(abs(v) for v in t["lo"]) < 1e-45 and max(t["r2"]) < 1e-80
    gen = acc.generator()
    t = truth.solve("nview", *gen.track(2, 4, 0)[:1], gen.INTR, gen.track(2, 4, 0)[1])
    assert np.all(np.abs(t["lo"]) <= 0.5 * np.spacing(np.abs(t["hi"]))) and np.any(np.array(t["lo"]) != 0.0)
