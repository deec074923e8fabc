"""The hard matrices of the cheirality stage (mvgx_relative_pose_from_essential, openmvg_amd/csrc/mvgx_relative_pose.h), shared by
tests/test_relative_pose_hard_emu_cpu.py (the device code under the HIP emulation), tests/test_relative_pose_hard_gpu.py (-m gpu) and
tests/test_relative_pose_truth_cpu.py: families of E on which the kernel's own Jacobi iteration, its three conditional column swaps and
its cross-product completion of U and V take paths that the general motions of tests/_relative_pose_ref.general_motion never reach,
against the 50-digit decomposition of tests/_relative_pose_truth.py.

Every pair has N = 24 correspondences (one full row of 16 lanes and a ragged second one; the lane edges are the business of
tests/_relative_pose_cases.py). A family is one batch per triangulation method.

  pure-translation   R = I with t = +-e1, +-e2, +-e3 and a generic t: E is antisymmetric, +-e1 / +-e2 put a zero column first / second
  aligned            0.2 rad about e_k with t along e_k and along e_(k+1)
  angle              ANGLES about a random axis inside a cone of about 0.3 rad around the optical axis (so that the points in front of
                     the first camera can be in front of the second one at a half turn too - the generator asserts that they are)
  estimated          E + s N, N standard normal, s in NOISE, unscaled; the truth is the decomposition of the perturbed E
  scale              one generic E times 2^k, k in SCALE_K: a power of two changes no mantissa, and the kernel iterates on E times the
                     power of two that brings its largest entry to [1, 2), so the outputs are those of the unscaled pair BIT FOR BIT
                     (an iteration on E as given passes this in IEEE arithmetic only: the device's sqrt and division expansions do
                     not commute with the scaling to the last bit)
  extreme-scale      k in EXTREME_K: E^T E overflows or vanishes in double; the kernel scales its working copy of E by the power of two
                     that brings the largest entry to [1, 2), so the pose is that of the unscaled pair (compared to tolerance)
  offsets            three pairs of `angle` in a batch with start[0] = 5 and use_start[0] = 3, one list with every position twice, one
                     of 40 entries drawn with replacement from 24

Decision margins. The truth alone has every in-front margin and every ratio margin above MARGIN on every pair of every family (the
seeds were chosen so; tests/test_relative_pose_truth_cpu.py asserts it): NO case is left out of any comparison.

Tolerances. Per family, the error of the float64 restatement (tests/_relative_pose_ref.py, LAPACK's SVD) against the truth, over the
four methods: pose entries absolute (R, t, centre, entries of order 1), points relative to max(1, |X|). Printed by
    python -m tests._relative_pose_hard_cases
and written down in SPREAD below. The kernel's tolerance is 1000 x that spread - the project's usual margin between "differs by
rounding" and "differs" - and never below 1000 x 2^-52. The spread is the restatement's, never the kernel's.
"""
import functools

import numpy as np

from openmvg_amd import _capi
from openmvg_amd import relative_pose as rp
from tests import _relative_pose_cases as base
from tests import _relative_pose_ref as rref
from tests import _relative_pose_truth as truth

N = 24
SEED = 20261022
MARGIN = 1e-6
RATIO = 0.7
ANGLES = (1e-9, 1e-6, 1e-3, 1.0, 2.0, 3.0, np.pi - 1e-9, np.pi)
NOISE = (1e-12, 1e-6, 1e-3, 1e-2)
SCALE_K = (-60, -20, 20, 60)
EXTREME_K = (-600, -300, 300, 600)
OFFSET_PAIRS = (3, 5, 7)   # of `angle`: 1 rad, 3 rad, a half turn
FAMILIES = ("pure-translation", "aligned", "angle", "estimated", "scale", "extreme-scale", "offsets")

# (pose, points): the restatement against the truth, as `python -m tests._relative_pose_hard_cases` printed them
# (none is more than 100 x the 1.6e-15 of the existing fixture: these matrices are hard for an iteration's control flow, not for the
# conditioning of R and t - the gap between the second and third singular value stays near 1 / sqrt(2) of the norm throughout)
SPREAD = {
    "pure-translation": (2.220446049250313e-16, 5.7927540864022036e-15),
    "aligned": (4.163336342344337e-16, 1.9601887304036662e-14),
    "angle": (8.881784197001252e-16, 2.124156053041542e-14),
    "estimated": (8.881784197001252e-16, 4.28259927939092e-15),
    "scale": (4.0245584642661925e-16, 1.5244946405799512e-15),
    "extreme-scale": (2.7755575615628914e-16, 4.791173575782201e-15),
    "offsets": (8.881784197001252e-16, 6.995463868240561e-15),
}
FLOOR = 2.0 ** -52


def tolerances(family):
    return tuple(1000.0 * max(s, FLOOR) for s in SPREAD[family])


# ---- the generators ----
def _pair(key, R, t, rng, E=None):
    """24 points in front of both cameras of (R, t) - asserted here, not assumed - and their noise-free bearings"""
    X = np.zeros((0, 3))
    for _ in range(200):
        c = np.stack([rng.uniform(-2, 2, 64), rng.uniform(-2, 2, 64), rng.uniform(2, 8, 64)], axis=1)
        X = np.concatenate([X, c[(c @ R.T + t)[:, 2] > 1.0]])[:N]
        if len(X) == N:
            break
    assert len(X) == N and (X[:, 2] >= 2.0).all() and ((X @ R.T + t)[:, 2] > 1.0).all(), key
    bI, bJ = rref.bearings(R, t, X)
    return dict(key=key, E=rref.essential(R, t) if E is None else E, bI=bI, bJ=bJ, use=None, R=R, t=t)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _generic_t(rng):
    return _unit(rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3))


@functools.lru_cache(maxsize=None)
def family(name):
    """the pairs of one family (drawn once; the four methods share them)"""
    rng = np.random.default_rng([SEED, FAMILIES.index(name)])
    eye, e = np.eye(3), np.eye(3)
    if name == "pure-translation":
        out = [_pair((name, k, int(s)), eye, s * e[k], rng) for k in range(3) for s in (1.0, -1.0)] + [_pair((name, "generic"), eye, _generic_t(rng), rng)]
        assert not out[0]["E"][:, 0].any() and not out[1]["E"][:, 0].any() and not out[2]["E"][:, 1].any() and not out[3]["E"][:, 1].any()   # the zero columns
        assert all(np.array_equal(p["E"], -p["E"].T) for p in out)
        return out
    if name == "aligned":
        return [_pair((name, k, j), rref.rotation(0.2 * e[k]), e[(k + j) % 3], rng) for k in range(3) for j in (0, 1)]
    if name == "angle":
        out = []
        for a in ANGLES:
            axis = _unit(e[2] + 0.3 * rng.standard_normal(3) / np.sqrt(3.0))
            out.append(_pair((name, a), rref.rotation(axis * a), _generic_t(rng), rng))
        return out
    if name == "estimated":
        out = []
        for s in NOISE:
            R, t = rref.general_motion(rng)
            out.append(_pair((name, s), R, t, rng, rref.essential(R, t) + s * rng.standard_normal((3, 3))))
        return out
    if name in ("scale", "extreme-scale"):
        R, t = rref.general_motion(rng)
        p0 = _pair((name, 0), R, t, rng)
        return [p0] + [dict(p0, key=(name, k), E=np.ldexp(p0["E"], k)) for k in (SCALE_K if name == "scale" else EXTREME_K)]
    assert name == "offsets"
    a = [dict(family("angle")[i]) for i in OFFSET_PAIRS]
    a[0]["use"] = rng.permutation(np.repeat(np.arange(N), 2)).astype(np.uint32)    # every position twice
    a[1]["use"] = rng.integers(0, N, 40).astype(np.uint32)                         # longer than the pair, drawn with replacement
    a[2]["use"] = rng.permutation(N)[:17].astype(np.uint32)
    assert len(set(a[1]["use"].tolist())) < 40 <= len(a[1]["use"])
    return [dict(p, key=("offsets",) + p["key"][1:]) for p in a]


@functools.lru_cache(maxsize=None)
def truths(name, method):
    return [truth.relative_pose_from_essential(p["bI"], p["bJ"], p["E"], p["use"], RATIO, method) for p in family(name)]


@functools.lru_cache(maxsize=None)
def restatements(name, method):
    return [rref.relative_pose_from_essential(p["bI"], p["bJ"], p["E"], p["use"], RATIO, method) for p in family(name)]


def pose_of(r):
    return np.concatenate([r.R.ravel(), r.t, r.center])


def point_error(points, ref):
    return float((np.abs(points - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))).max()) if len(ref) else 0.0


def measure_spread(name):
    """(pose, points): the restatement against the truth over the four methods - decisions equal, or there is nothing to measure"""
    pose = points = 0.0
    for method in range(4):
        for p, own, tr in zip(family(name), restatements(name, method), truths(name, method)):
            assert own.ok == tr.ok and tr.ok and sorted(own.cheirality) == sorted(tr.cheirality) and np.array_equal(own.selected, tr.selected), (p["key"], method)
            pose = max(pose, float(np.abs(pose_of(own) - pose_of(tr)).max()))
            points = max(points, point_error(own.points, tr.points))
    return pose, points


# ---- the checks ----
def check_margins(name, method):
    for p, tr in zip(family(name), truths(name, method)):
        assert tr.point_margin > MARGIN and tr.ratio_margin > MARGIN, (p["key"], method, tr.point_margin, tr.ratio_margin)


def _call(name, method, **over):
    cases = [dict(p, method=method, ratio=RATIO) for p in family(name)]
    rc, out = base.call_from_essential(cases, any(c["use"] is not None for c in cases), **over)
    assert rc == _capi.MVGX_OK, _capi.lib().mvgx_last_error()
    ss = out["sel_start"]
    assert int(ss[0]) == 0 and (np.diff(ss.astype(np.int64)) >= 0).all()
    assert base.untouched(out, len(cases), int(ss[-1])), "the call wrote behind its lists or results"
    return cases, out


def check_against_truth(name, method):
    """one batch of the family on the library _capi is routed to, every pair against the 50-digit truth; -> the cases and the call's outputs"""
    cases, out = _call(name, method)
    tol_pose, tol_points = tolerances(name)
    ss = out["sel_start"]
    for p, (c, tr) in enumerate(zip(cases, truths(name, method))):
        key, row = (c["key"], method), out["res"][p]
        assert tr.point_margin > MARGIN and tr.ratio_margin > MARGIN, key   # (no case is left out: the seeds keep every margin)
        lo, hi = int(ss[p]), int(ss[p + 1])
        selected, points = out["sel"][lo:hi], out["X"][lo:hi]
        counts = tuple(int(v) for v in row["cheirality"])
        assert np.array_equal(row["E"], np.asarray(c["E"]).reshape(9)), key
        assert bool(row["ok"]) == tr.ok and tr.ok, (key, row["ok"], counts, tr.cheirality)
        # two decompositions differ by signs of (u_i, v_i) pairs and by the basis of an equal plane: A = u2 v1^T - u1 v2^T and u3 change sign
        # TOGETHER or not at all, so the candidates come in the truth's order or with 0 <-> 1 and 2 <-> 3 exchanged (include/mvgx.h) - never otherwise
        assert counts in (tr.cheirality, tuple(tr.cheirality[i] for i in (1, 0, 3, 2))), (key, counts, tr.cheirality)
        assert int(row["n_selected"]) == max(counts) == hi - lo, (key, row["n_selected"], counts)
        assert np.array_equal(selected, tr.selected), key
        Rt = row["pose"][:12].reshape(3, 4)
        d_pose = float(np.abs(np.concatenate([Rt[:, :3].ravel(), Rt[:, 3], row["pose"][12:]]) - pose_of(tr)).max())
        assert d_pose <= tol_pose, (key, d_pose, tol_pose)
        d_pts = point_error(points, tr.points)
        assert d_pts <= tol_points, (key, d_pts, tol_points)
    return cases, out


def _same_outputs(out, p, q, key):
    """pair p's pose, counts, list and points are pair q's, bit for bit"""
    for f in ("pose", "cheirality", "n_selected", "ok", "found_precision", "n_acransac_inliers"):
        assert out["res"][p][f].tobytes() == out["res"][q][f].tobytes(), (key, f)
    ss = out["sel_start"].astype(np.int64)
    assert np.array_equal(out["sel"][ss[p]:ss[p + 1]], out["sel"][ss[q]:ss[q + 1]]) and out["X"][ss[p]:ss[p + 1]].tobytes() == out["X"][ss[q]:ss[q + 1]].tobytes(), key


def check_scale(method):
    cases, out = check_against_truth("scale", method)
    for p in range(1, len(cases)):
        _same_outputs(out, p, 0, (cases[p]["key"], method))


def check_extreme_scale(method):
    check_against_truth("extreme-scale", method)


def check_no_motion(method):
    """a zero E and E with entries that are not finite - everywhere, in the third column alone, in one entry of the first: ok = 0, a zero
    pose, nothing listed; the ordinary pair beside them is untouched by their company"""
    p0 = family("scale")[0]
    nan3, inf1 = p0["E"].copy(), p0["E"].copy()
    nan3[:, 2] = np.nan
    inf1[1, 0] = np.inf
    cases = [dict(p0, E=E, method=method, ratio=RATIO) for E in (np.zeros((3, 3)), np.full((3, 3), np.nan), nan3, inf1, -inf1, p0["E"])]
    with np.errstate(all="ignore"):
        rc, out = base.call_from_essential(cases, False)
    assert rc == _capi.MVGX_OK, _capi.lib().mvgx_last_error()
    for p in range(5):
        row = out["res"][p]
        assert row["ok"] == 0 and not row["pose"].any() and row["n_selected"] == 0 and int(out["sel_start"][p + 1]) == 0, (p, method, row)
        assert not row["cheirality"].any(), (p, method, row["cheirality"])
        assert row["E"].tobytes() == np.asarray(cases[p]["E"]).tobytes(), p
    assert out["res"][5]["ok"] == 1 and int(out["sel_start"][6]) == int(out["res"][5]["n_selected"]) == N
    assert base.untouched(out, len(cases), N)


def check_offsets(method):
    """the batch addressed from start[0] = 5 and use_start[0] = 3, rows and entries in front that belong to nobody: the results of the
    same pairs called from 0, and lists that repeat positions exactly as listed"""
    cases, plain = check_against_truth("offsets", method)
    n_corr, n_list = N * len(cases), sum(len(c["use"]) for c in cases)
    start = (5 + N * np.arange(len(cases) + 1)).astype(np.uint64)
    use_start = (3 + np.concatenate([[0], np.cumsum([len(c["use"]) for c in cases])])).astype(np.uint64)
    front = np.full((5, 3), np.nan)   # whoever reads a row in front of start[0] is poisoned by it
    bI = np.ascontiguousarray(np.concatenate([front] + [c["bI"] for c in cases] + [np.zeros((1, 3))]))
    bJ = np.ascontiguousarray(np.concatenate([front] + [c["bJ"] for c in cases] + [np.zeros((1, 3))]))
    use_index = np.ascontiguousarray(np.concatenate([np.full(3, 0xFFFFFFFF, np.uint32)] + [c["use"] for c in cases] + [np.zeros(1, np.uint32)]))
    assert len(bI) == 5 + n_corr + 1 and len(use_index) == 3 + n_list + 1
    _, moved = _call("offsets", method, start=start, bI=bI, bJ=bJ, use_start=use_start, use_index=use_index)
    assert np.array_equal(moved["sel_start"], plain["sel_start"]) and np.array_equal(moved["sel"], plain["sel"]) and moved["X"].tobytes() == plain["X"].tobytes()
    for p in range(len(cases)):
        assert all(moved["res"][p][f].tobytes() == plain["res"][p][f].tobytes() for f in rp._RESULT.names), (p, method)
    # repeats: the list of the winner is the pair's list with the positions behind a camera struck out, nothing merged
    ss = plain["sel_start"].astype(np.int64)
    for p, c in enumerate(cases):
        sel = plain["sel"][ss[p]:ss[p + 1]]
        in_front = set(sel.tolist())
        assert np.array_equal(sel, [u for u in c["use"] if int(u) in in_front]), (p, method)
    assert int(plain["res"][0]["n_selected"]) == 2 * N and int(plain["res"][1]["n_selected"]) == 40   # noise-free pairs: every listed entry is in front


CHECKS = {"scale": check_scale, "extreme-scale": check_extreme_scale, "offsets": check_offsets}


def check_family(name, method):
    if name in CHECKS:
        CHECKS[name](method)
    else:
        check_against_truth(name, method)


if __name__ == "__main__":
    for fam in FAMILIES:
        print(fam, measure_spread(fam), flush=True)
