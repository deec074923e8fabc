"""CPU, no library: the 50-digit yardstick of the relative pose (tests/_relative_pose_truth.py) against what the suite already trusts -
the float64 restatement (tests/_relative_pose_ref.py) and the compiled reference's fixture rows (tests/golden/relative_pose_golden.npz)
on the 64 cases of the stage -, the decision margins of the hard families (tests/_relative_pose_hard_cases.py), the recorded spreads,
and the module's own independence of the basis it draws inside a plane of equal singular values."""
import numpy as np
import pytest
from mpmath import mp, mpf

from tests import _relative_pose_hard_cases as hard
from tests import _relative_pose_ref as rref
from tests import _relative_pose_truth as truth
from tests import _relative_pose_cases as base


@pytest.mark.parametrize("method", range(4))
def test_truth_against_restatement_and_compiled_reference(method):
    """decisions equal on every case of the method (the guard of the fixture excuses none here), pose within the existing TOL_POSE"""
    tol_pose, tol_points = base.tolerances()
    n = 0
    for key, c in base.stage_cases().items():
        if c["method"] != method:
            continue
        n += 1
        c = dict(c, key=key, ok=c["ref_ok"], counts=c["ref_counts"], pose=c["ref_pose"], selected=c["ref_selected"], points=c["ref_points"])
        tr = truth.relative_pose_from_essential(c["bI"], c["bJ"], c["E"], c["use"], c["ratio"], method)
        own = rref.relative_pose_from_essential(c["bI"], c["bJ"], c["E"], c["use"], c["ratio"], method)
        assert tr.ok == c["ok"] == own.ok and sorted(tr.cheirality) == sorted(c["counts"]) == sorted(own.cheirality), (c["key"], tr.cheirality, c["counts"])
        if not tr.ok:
            continue
        assert np.array_equal(tr.selected, c["selected"]) and np.array_equal(tr.selected, own.selected), c["key"]
        for other in (c["pose"], hard.pose_of(own)):
            assert np.abs(hard.pose_of(tr) - other).max() <= tol_pose, c["key"]
        for other in (c["points"], own.points):
            assert hard.point_error(other, tr.points) <= tol_points, c["key"]
    assert n == 16


@pytest.mark.parametrize("family", hard.FAMILIES)
def test_every_margin_of_the_hard_families_is_wide(family):
    """the truth alone: no in-front test and no ratio within 1e-6 of flipping, on any pair under any method - the hard-case tests leave
    out nothing, and a change of seed cannot make them"""
    for method in range(4):
        hard.check_margins(family, method)
        assert all(tr.ok for tr in hard.truths(family, method))


@pytest.mark.parametrize("family", hard.FAMILIES)
def test_recorded_spreads_are_the_restatements(family):
    """SPREAD holds what the restatement gives against the truth (to the order: another LAPACK build may round another way)"""
    pose, points = hard.measure_spread(family)
    assert pose <= 10.0 * max(hard.SPREAD[family][0], hard.FLOOR) and points <= 10.0 * max(hard.SPREAD[family][1], hard.FLOOR), (family, pose, points)
    assert hard.SPREAD[family][0] <= 100.0 * 1.6e-15   # (above that the cases module owes an explanation by conditioning)


def test_families_hold_their_constructions():
    assert [len(hard.family(f)) for f in hard.FAMILIES] == [7, 6, 8, 4, 5, 5, 3]
    assert all(len(p["bI"]) == hard.N == 24 for f in hard.FAMILIES for p in hard.family(f))
    # equal singular values where the issue expects them exact: the integer matrices [+-e_k]x
    eq = [tr.equal_singular_values for tr in hard.truths("pure-translation", 3)]
    assert all(eq[:6])
    s = hard.family("scale")
    assert all(np.array_equal(p["E"], s[0]["E"] * 2.0 ** k) for p, k in zip(s[1:], hard.SCALE_K))
    x = hard.family("extreme-scale")
    assert all(np.isfinite(p["E"]).all() and np.array_equal(np.ldexp(p["E"], -k), x[0]["E"]) for p, k in zip(x[1:], hard.EXTREME_K))
    R = hard.family("angle")[-1]["R"]
    assert np.abs(R - R.T).max() < 1e-14   # a half turn: R is symmetric (to the rounding of sin(pi) and of the Rodrigues products)


def test_truth_does_not_depend_on_the_basis_of_an_equal_plane():
    """the module's own check ran (sigma_1 = sigma_2 to 40 digits) and held, on an antisymmetric E, a half turn and the zero-column
    matrices; and a basis turned by any other angle gives the same rotations"""
    E = [np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]),
         np.array([[0.0, -3.0, 2.0], [3.0, 0.0, -6.0], [-2.0, 6.0, 0.0]]),                     # [t]x, t = (6, 2, 3): |t| = 7
         np.array([[0.0, -3.0, 2.0], [3.0, 0.0, -6.0], [-2.0, 6.0, 0.0]]) @ np.diag([-1.0, -1.0, 1.0])]   # ... times a half turn about e3
    with mp.workdps(truth.DPS):
        for M in E:
            report = {}
            R0, R1, u3 = truth.motion_from_essential(M, report)
            assert report["equal"] and report["basis_error"] < 1e-40, report
            for R in (R0, R1):   # rotations, and E = +-[u3]x R up to scale
                RtR = [[sum(R[k][i] * R[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
                assert max(abs(RtR[i][j] - (1 if i == j else 0)) for i in range(3) for j in range(3)) < mpf(10) ** -40
                tx = [[0, -u3[2], u3[1]], [u3[2], 0, -u3[0]], [-u3[1], u3[0], 0]]
                P = [[sum(tx[i][k] * R[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
                big = max(abs(float(v)) for v in M.ravel())
                n = max(abs(P[i][j]) for i in range(3) for j in range(3))
                assert min(max(abs(P[i][j] / n - s * mpf(float(M[i, j])) / big) for i in range(3) for j in range(3)) for s in (1, -1)) < mpf(10) ** -40
    with pytest.raises(truth.NoMotion):
        with mp.workdps(truth.DPS):
            truth.motion_from_essential(np.zeros((3, 3)))
    assert not truth.relative_pose_from_essential(np.zeros((0, 3)), np.zeros((0, 3)), np.full((3, 3), np.nan)).ok
