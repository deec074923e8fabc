"""The essential-matrix model of the geometric filter (E_ACRobust.hpp:39-150; VERDICT r3 missing #1):
GeometricFilter_EMatrix_AC = ACKernelAdaptorEssential<FivePointSolver, EpipolarDistanceError> + ACRANSAC.
CPU: the five-point restatement and the emulated device solver against the reference's stored FivePointsRelativePose answers; the
restatement of the whole filter against the compiled reference's stored outputs (and live); the emulated kernel on a few pairs.
GPU: the device solver alone, the golden fixture, the compiled reference on mixed sizes - same parity policy as F / H
(tests/_geofilter_cases.py: identical inlier sets, then NFA / precision / model equal; the remainder bounded by the reference's own
build-to-build spread)."""
import ctypes as C
import os

import numpy as np
import pytest

from openmvg_amd import _capi, geofilter, synth
from tests import _emu, _geofilter_cases as gc, _oracle
from tests._adapter_route import device_route

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geofilter_e.npz"))
FUNCTOR = geofilter.GeometricFilter_EMatrix_AC


def _norm_e(E):
    E = np.asarray(E, np.float64).reshape(9)
    E = E / np.linalg.norm(E)
    return E * np.sign(E[np.abs(E).argmax()])


def _five_point(fn, b1, b2):
    Es = np.zeros(90); n = C.c_int(0)
    rc = fn(np.ascontiguousarray(b1).ctypes.data_as(C.c_void_p), np.ascontiguousarray(b2).ctypes.data_as(C.c_void_p), Es.ctypes.data_as(C.c_void_p), C.byref(n))
    assert rc in (0, None), rc
    return [_norm_e(Es[9 * k:9 * k + 9]) for k in range(n.value)]


def _check_five_point(fn, tol, sel=None):
    """every stored reference solution is found (same count, essential matrices equal after normalisation)"""
    worst = 0.0
    for t in (range(len(GOLD["fp_n"])) if sel is None else sel):
        want = [_norm_e(GOLD["fp_E"][t][k]) for k in range(int(GOLD["fp_n"][t]))]
        got = _five_point(fn, GOLD["fp_b1"][t], GOLD["fp_b2"][t])
        assert len(got) == len(want), (t, len(got), len(want))
        for w in want:
            d = min(np.abs(w - g).max() for g in got)
            worst = max(worst, d)
            assert d < tol, (t, d)
    return worst


def test_five_point_restatement_reproduces_the_reference_solutions():
    lib = _oracle.port()
    lib.port_five_point.restype = None
    _check_five_point(lib.port_five_point, 1e-7)


def test_five_point_emulated_device_solver_reproduces_the_reference_solutions():
    """mvgx_debug_five_point (test hook): the wave-level solver of openmvg_amd/csrc/geofilter_five_point.h under the HIP emulation"""
    h = _emu.handle()
    h.mvgx_debug_five_point.restype = C.c_int
    _check_five_point(h.mvgx_debug_five_point, 1e-7, sel=range(24))


def _five_point4_equals_four_solves(h, tests):
    """mvgx_debug_five_point4 (solve4: four samples, one per 16-lane row) == mvgx_debug_five_point on each sample, bit for bit"""
    h.mvgx_debug_five_point.restype = C.c_int
    h.mvgx_debug_five_point4.restype = C.c_int
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    nt = len(GOLD["fp_n"])
    total = 0
    for t0 in range(0, tests, 4):
        idx = [min(t0 + k, nt - 1) for k in range(4)]
        b1 = np.ascontiguousarray(np.stack([GOLD["fp_b1"][t] for t in idx]), np.float64)
        b2 = np.ascontiguousarray(np.stack([GOLD["fp_b2"][t] for t in idx]), np.float64)
        E4 = np.zeros(360); n4 = (C.c_int * 4)()
        assert h.mvgx_debug_five_point4(P(b1), P(b2), P(E4), n4) == 0
        for k, t in enumerate(idx):
            E1 = np.zeros(90); n1 = C.c_int(0)
            assert h.mvgx_debug_five_point(P(np.ascontiguousarray(b1[k])), P(np.ascontiguousarray(b2[k])), P(E1), C.byref(n1)) == 0
            assert n1.value == n4[k], (t, n1.value, n4[k])
            assert np.array_equal(E1[:9 * n1.value], E4[90 * k:90 * k + 9 * n1.value]), (t, np.abs(E1[:9 * n1.value] - E4[90 * k:90 * k + 9 * n1.value]).max())
            total += n1.value
    assert total > tests   # (more than one solution per sample on average)


def test_five_point_four_samples_per_wave_equal_the_one_sample_solver_emulated():
    _five_point4_equals_four_solves(_emu.handle(), 24)


def _samples_ahead_equal_one_sample_per_iteration(tv, K, b, max_iterations, aheads=("4", "3")):
    """MVGX_GEO_AHEAD=1 (one five-point solve per a-contrario iteration) against samples drawn and solved ahead: every output equal"""
    saved = os.environ.get("MVGX_GEO_AHEAD")
    out = {}
    try:
        for ahead in ("1",) + tuple(aheads):
            os.environ["MVGX_GEO_AHEAD"] = ahead
            mask, res, st = geofilter.filter_pairs_e(tv["xI"], tv["xJ"], tv["start"], tv["wh"], K, FUNCTOR(4.0, max_iterations), bearings=b)
            out[ahead] = (mask.copy(), res.copy(), int(st.n_iterations), int(st.n_models), int(st.n_pairs_ok))
    finally:
        if saved is None:
            os.environ.pop("MVGX_GEO_AHEAD", None)
        else:
            os.environ["MVGX_GEO_AHEAD"] = saved
    one = out["1"]
    for ahead in aheads:
        got = out[ahead]
        assert got[2:] == one[2:], (ahead, got[2:], one[2:])
        assert np.array_equal(got[0], one[0]) and got[1].tobytes() == one[1].tobytes(), ahead
    return one


def test_samples_ahead_equal_one_sample_per_iteration_emulated():
    """a pair the filter accepts and one it rejects, 2 048 iterations: the warm-up, the change of mode, pool rebuilds, a twist of the
    generator inside a batch of samples (revoked draw) - all on the path"""
    start = GOLD["start"].astype(np.int64)
    n = np.diff(start)
    small = [int(p) for p in np.argsort(n) if 12 < n[p] <= 60]
    sel = [p for p in small if GOLD["ok"][p]][:2] + [p for p in small if not GOLD["ok"][p]][:1]
    tv, ref, K, b = _gold_tv(sel)
    with _emu.emulated():
        one = _samples_ahead_equal_one_sample_per_iteration(tv, K, b, 2048)
    assert one[2] > 300 and one[4] == 2   # (several twists of the 624-word state: ~5 draws per iteration)


def _gold_tv(sel=None):
    start = GOLD["start"].astype(np.int64)
    pairs = list(range(len(start) - 1)) if sel is None else list(sel)
    cut = lambda a: np.concatenate([a[start[p]:start[p + 1]] for p in pairs])   # noqa: E731
    tv = dict(xI=cut(GOLD["xI"]), xJ=cut(GOLD["xJ"]), wh=GOLD["wh"][pairs],
              start=np.concatenate([[0], np.cumsum([start[p + 1] - start[p] for p in pairs])]).astype(np.uint64))
    ref = dict(mask=cut(GOLD["mask"]), ok=GOLD["ok"][pairs], F=GOLD["F"][pairs], precision=GOLD["precision"][pairs], nfa=GOLD["nfa"][pairs])
    return tv, ref, GOLD["K"][pairs], (cut(GOLD["bI"]), cut(GOLD["bJ"]))


def test_restatement_equals_the_stored_reference_outputs():
    tv, ref, K, b = _gold_tv()
    got = _oracle.port_geofilter_e(tv, K, bearings=b)
    differing, rep = gc.compare(tv["start"], ref, got["mask"], got["ok"], got["F"], got["precision"], got["nfa"])
    assert rep["pairs_ok_reference"] > 100 and len(differing) <= gc.allowed_differing(rep["pairs"], "e"), (rep, differing)


@pytest.mark.skipif(not _oracle.have_ref_geofilter(), reason="oracle/_ref/libref_geofilter.so not built (needs /root/reference)")
def test_restatement_equals_the_compiled_reference_live():
    tv = synth.two_view_matches(300, seed=78, n_max=200)
    K = synth.two_view_calibration(tv)
    b = _oracle.ref_pinhole_bearings(tv, K)
    for iters in (2048, 40):
        ref = _oracle.ref_geofilter_e(tv, K, max_iterations=iters)
        got = _oracle.port_geofilter_e(tv, K, max_iterations=iters, bearings=b)
        differing, rep = gc.compare(tv["start"], ref, got["mask"], got["ok"], got["F"], got["precision"], got["nfa"])
        assert len(differing) <= gc.allowed_differing(rep["pairs"], "e"), (iters, rep, differing)


def test_host_bearings_equal_the_reference_cameras_to_rounding():
    tv, _, K, (bI, bJ) = _gold_tv(range(20))
    st = tv["start"].astype(np.int64)
    for p in range(20):
        assert np.abs(geofilter.pinhole_bearings(K[p, 0], tv["xI"][st[p]:st[p + 1]]) - bI[st[p]:st[p + 1]]).max() < 1e-14 if st[p + 1] > st[p] else True


def test_emulated_device_code_equals_the_stored_reference_outputs():
    """the essential instantiation of the kernel under the HIP emulation on a few small golden pairs (one fiber per lane: slow)"""
    start = GOLD["start"].astype(np.int64)
    n = np.diff(start)
    small = [int(p) for p in np.argsort(n) if 12 < n[p] <= 60]
    sel = [p for p in small if GOLD["ok"][p]][:1] + [p for p in small if not GOLD["ok"][p]][:1] + [int(np.argmin(n))]
    tv, ref, K, b = _gold_tv(sel)
    with _emu.emulated():
        mask, res, st = geofilter.filter_pairs_e(tv["xI"], tv["xJ"], tv["start"], tv["wh"], K, FUNCTOR(4.0, 2048), bearings=b)
    differing, rep = gc.compare(tv["start"], ref, mask, res["ok"], res["F"], res["precision_robust"], res["nfa"])
    assert not differing, (rep, differing)
    assert int(st.n_pairs_ok) == int(ref["ok"].sum()) and int(st.n_models) >= int(st.n_iterations) > 0


def test_argument_errors_under_emulation():
    with _emu.emulated():
        xI = np.zeros((3, 2)); start = np.array([0, 3], np.uint64); wh = np.array([[100, 100, 100, 100]], np.uint32)
        K = np.tile(np.array([[90.0, 0, 50], [0, 90.0, 50], [0, 0, 1]]), (1, 2, 1, 1))
        mask, res, st = geofilter.filter_pairs_e(xI, xI, start, wh, K)   # fewer than 6 correspondences: rejected without estimation
        assert not mask.any() and not res["ok"][0] and np.array_equal(res["F"][0], np.eye(3))
        with pytest.raises(ValueError):
            geofilter.filter_pairs_e(xI, xI, start, wh, K[:0])


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.mark.gpu
def test_five_point_device_solver_reproduces_the_reference_solutions():
    lib = _capi.lib()
    lib.mvgx_debug_five_point.restype = C.c_int
    worst = _check_five_point(lib.mvgx_debug_five_point, 1e-7)
    assert worst < 1e-7


@pytest.mark.gpu
def test_five_point_four_samples_per_wave_equal_the_one_sample_solver():
    _five_point4_equals_four_solves(_capi.lib(), len(GOLD["fp_n"]))


@pytest.mark.gpu
def test_samples_ahead_equal_one_sample_per_iteration_on_the_device():
    tv, ref, K, b = _gold_tv()
    _samples_ahead_equal_one_sample_per_iteration(tv, K, b, 2048, aheads=("4", "2"))
    _samples_ahead_equal_one_sample_per_iteration(tv, K, b, 37, aheads=("4",))
    big = synth.two_view_matches(120, seed=4711, n_max=14000)   # every size class, global-table class included
    Kb = synth.two_view_calibration(big)
    _samples_ahead_equal_one_sample_per_iteration(big, Kb, None, 1024, aheads=("4",))


@pytest.mark.gpu
def test_golden_fixture_inlier_sets_on_the_device():
    tv, ref, K, b = _gold_tv()
    mask, res, st = geofilter.filter_pairs_e(tv["xI"], tv["xJ"], tv["start"], tv["wh"], K, FUNCTOR(4.0, 2048), bearings=b)
    differing, rep = gc.compare(tv["start"], ref, mask, res["ok"], res["F"], res["precision_robust"], res["nfa"])
    assert rep["pairs_ok_reference"] > 100 and len(differing) <= gc.allowed_differing(rep["pairs"], "e"), (rep, differing)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,iters", [(dict(seed=15, n_max=400), 2048), (dict(seed=16, n_max=120, inlier_frac=(0.15, 0.5)), 1024),
                                      (dict(seed=17, n_max=200), 37), (dict(seed=18, n_min=1100, n_max=1300, tiny_frac=0.0), 2048)])
def test_against_the_compiled_reference(kw, iters):
    if not _oracle.have_ref_geofilter():
        pytest.skip("oracle/_ref/libref_geofilter.so not built")
    n_pairs = 40 if kw.get("n_min", 0) > 1000 else 800
    tv = synth.two_view_matches(n_pairs, **kw)
    K = synth.two_view_calibration(tv)
    ref = _oracle.ref_geofilter_e(tv, K, 4.0, iters)
    b = _oracle.ref_pinhole_bearings(tv, K)
    mask, res, _ = geofilter.filter_pairs_e(tv["xI"], tv["xJ"], tv["start"], tv["wh"], K, FUNCTOR(4.0, iters), bearings=b)
    differing, rep = gc.compare(tv["start"], ref, mask, res["ok"], res["F"], res["precision_robust"], res["nfa"])
    assert len(differing) <= gc.allowed_differing(rep["pairs"], "e"), (rep, differing[:10])


@pytest.mark.gpu
def test_host_bearings_give_the_same_inlier_sets_as_the_reference_cameras():
    """filter_pairs_e with bearings=None (numpy Kinv) against bearings from the reference's camera class"""
    tv, ref, K, b = _gold_tv(range(120))
    m1, r1, _ = geofilter.filter_pairs_e(tv["xI"], tv["xJ"], tv["start"], tv["wh"], K, FUNCTOR(4.0, 2048), bearings=b)
    m2, r2, _ = geofilter.filter_pairs_e(tv["xI"], tv["xJ"], tv["start"], tv["wh"], K, FUNCTOR(4.0, 2048))
    st = tv["start"].astype(np.int64)
    diff = sum(1 for p in range(120) if not np.array_equal(m1[st[p]:st[p + 1]], m2[st[p]:st[p + 1]]))
    assert diff <= gc.allowed_differing(120, "e")


# ---- the drop-in: ImageCollectionGeometricFilter::Robust_model_estimation<GeometricFilter_EMatrix_AC> ----
def _container_case(kind, guided=False, monkeypatch=None):
    """a collection of calibrated pairs (every view but the last has a Pinhole_Intrinsic: the pairs of the last view take the functor's
    "no intrinsic information" branch) through the same caller, linked against the reference template or the adapter's specialisation.
    With `monkeypatch` the call runs under the route check: the device pairs are those whose two views have a pinhole intrinsic, and
    (guided) every accepted one of them is guided on the device (SIFT rows)"""
    from tests import _geofilter_scene
    feats, wh, putative = _geofilter_scene.collection(n_pairs=5, seed=12, n_min=40, n_max=70, inlier_frac=(0.6, 0.9), no_geometry_frac=0.2, size=(1000, 1000))
    run = lambda: _oracle.geofilter_container(kind, feats, wh, putative, max_iterations=512, guided=guided, model="e", focal=900.0)   # noqa: E731
    if monkeypatch is None:
        return run()
    last = len(feats) - 1
    on_device = [k for k in putative if last not in k]
    got = {}
    with device_route(_oracle.geofilter_container_lib(kind), len(on_device), monkeypatch,
                      guided=(lambda: (sum(k in got for k in on_device), 0)) if guided else None):
        got.update(run())
    return got


def test_adapter_specialisation_fills_the_container_like_the_reference_template(monkeypatch):
    if _oracle.geofilter_container_lib("reference") is None or _oracle.geofilter_container_lib("adapter_emu") is None:
        pytest.skip("needs /root/reference (reference library and adapter harness)")
    want, got = _container_case("reference"), _container_case("adapter_emu", monkeypatch=monkeypatch)
    assert set(want) == set(got) and len(want) >= 2 and (8, 9) not in want   # (the pair of the view without intrinsics is rejected by both)
    assert all(np.array_equal(want[k], got[k]) for k in want)


@pytest.mark.gpu
@pytest.mark.parametrize("guided", [False, True])
def test_adapter_specialisation_on_the_device(guided, monkeypatch):
    if _oracle.geofilter_container_lib("reference") is None or _oracle.geofilter_container_lib("adapter") is None:
        pytest.skip("adapter harness / reference library not present")
    want, got = _container_case("reference", guided), _container_case("adapter", guided, monkeypatch)
    assert set(want) == set(got) and len(want) >= 2
    assert all(np.array_equal(want[k], got[k]) for k in want)
