"""Inputs and checks of the geometric filter's entries and launch forms at the edges of its size classes, for each of the six models
(F, H, E, the two angular E, orthographic E). Shared by the GPU test and by the CPU test that runs the same source under the HIP emulation.

One call per model carries pairs of m, 0, m + 1, 9, 64, 65, 256 and 257 correspondences (m = the model's minimal sample; `limit` cuts the
list for the emulation): not estimated | empty | the smallest estimated | one wave's round of residuals and one more | the largest pair
whose tables live in LDS and the smallest whose tables live in global scratch. 48 iterations. Synthetic two-view pairs of
openmvg_amd/synth.py with fixed seeds; bearing vectors by the host mirror of the pinhole camera, calibration matrices of the synthetic
cameras, the orthographic model's inputs by geofilter.ortho_inputs.

Checked, byte for byte (inlier mask, result records, iterations and models run):
  * the indexed entry == the gathered entry, the features of every image stored shuffled with unused ones in between
  * MVGX_GEO_GLOBAL_ABOVE=8 (tables in global scratch from nine correspondences on) == the default form
  * H and E: MVGX_GEO_AHEAD=1 (one minimal solve per iteration) == the default (four samples ahead)
  * pairs of at most m correspondences come back rejected, without inliers, with the identity model"""
import contextlib
import functools
import os

import numpy as np

from openmvg_amd import geofilter, synth
from tests import _emu

MODELS = ("f", "h", "e", "ea", "eu", "eo")
MIN_SAMPLE = {"f": 7, "h": 4, "e": 5, "ea": 8, "eu": 3, "eo": 3}
ITERATIONS = 48
PRECISION = {"f": 4.0, "h": 4.0, "e": 4.0, "ea": 4.0, "eu": 4.0, "eo": 2.0}   # pixels; degrees for the angular models
_ENTRY = {"f": "mvgx_geofilter_f_acransac", "h": "mvgx_geofilter_h_acransac", "e": "mvgx_geofilter_e_acransac", "ea": "mvgx_geofilter_e_angular_acransac",
          "eu": "mvgx_geofilter_e_angular_acransac", "eo": "mvgx_geofilter_eo_acransac"}


def sizes(model, limit=257):
    m = MIN_SAMPLE[model]
    return [m, 0] + [n for n in (m + 1, 9, 64, 65, 256, 257) if n <= limit]


@functools.lru_cache(maxsize=None)
def scene(model, limit=257):
    """the arrays of one call in both forms; never modified"""
    make = synth.two_view_homography_matches if model == "h" else synth.two_view_matches
    tvs = [make(1, seed=500 + 10 * k + MODELS.index(model), n_min=n, n_max=n, tiny_frac=0.0, no_geometry_frac=0.0) for k, n in enumerate(sizes(model, limit))]
    start = np.concatenate([[0], np.cumsum([len(t["xI"]) for t in tvs])]).astype(np.uint64)
    assert list(np.diff(start.astype(np.int64))) == sizes(model, limit)
    xI, xJ = np.concatenate([t["xI"] for t in tvs]), np.concatenate([t["xJ"] for t in tvs])
    wh = np.concatenate([t["wh"] for t in tvs]).astype(np.uint32)
    K = synth.two_view_calibration(dict(wh=wh))
    n_pairs = len(tvs)
    st = start.astype(np.int64)
    bI, bJ = np.zeros((len(xI), 3)), np.zeros((len(xJ), 3))
    for p in range(n_pairs):
        if st[p + 1] > st[p]:
            bI[st[p]:st[p + 1]] = geofilter.pinhole_bearings(K[p, 0], xI[st[p]:st[p + 1]])
            bJ[st[p]:st[p + 1]] = geofilter.pinhole_bearings(K[p, 1], xJ[st[p]:st[p + 1]])
    bound = np.zeros(n_pairs)
    if model == "eo":   # the pixel arrays carry the hnormalized bearing vectors
        xI, xJ, bound = geofilter.ortho_inputs(xI, xJ, start, K, PRECISION[model])
    # indexed form: images 2 p, 2 p + 1 hold the pair's features in shuffled order, plus three unused features each
    feat_xy, feat_b, fstart, ij = [], [], [0], np.zeros((len(xI), 2), np.uint32)
    for p in range(n_pairs):
        m = int(st[p + 1] - st[p])
        for im, (x, b) in enumerate(((xI, bI), (xJ, bJ))):
            slot = np.random.default_rng(1000 * im + p).permutation(m + 3)[:m]
            fx = np.full((m + 3, 2), 7.0); fb = np.tile([0.0, 0.0, 1.0], (m + 3, 1))
            fx[slot] = x[st[p]:st[p + 1]]; fb[slot] = b[st[p]:st[p + 1]]
            feat_xy.append(fx); feat_b.append(fb); fstart.append(fstart[-1] + m + 3)
            ij[st[p]:st[p + 1], im] = slot
    c = np.ascontiguousarray
    return dict(model=model, n_pairs=n_pairs, n_matches=len(xI), start=start, xI=c(xI), xJ=c(xJ), bI=c(bI), bJ=c(bJ), wh=c(wh), K=c(K.reshape(-1, 18)),
                bound=c(bound), feat_xy=c(np.concatenate(feat_xy)), feat_b=c(np.concatenate(feat_b)), fstart=np.asarray(fstart, np.uint64),
                wh_image=c(wh.reshape(-1, 2)), K_image=c(K.reshape(-1, 9)), pairs=np.arange(2 * n_pairs, dtype=np.uint32).reshape(-1, 2), ij=c(ij))


def call(s, indexed):
    """one call of the model's gathered or indexed entry -> (mask bytes, result bytes, iterations, models, result array)"""
    model, np_, ni = s["model"], s["n_pairs"], 2 * s["n_pairs"]
    upright = int(model == "eu")
    if indexed:
        head = {"f": [s["feat_xy"], s["fstart"], s["wh_image"], ni, s["pairs"], s["start"], s["ij"], np_],
                "e": [s["feat_xy"], s["feat_b"], s["fstart"], s["wh_image"], s["K_image"], ni, s["pairs"], s["start"], s["ij"], np_],
                "ea": [s["feat_b"], s["fstart"], ni, s["pairs"], s["start"], s["ij"], np_, upright],
                "eo": [s["feat_xy"], s["fstart"], s["wh_image"], ni, s["pairs"], s["start"], s["ij"], s["bound"], np_]}
    else:
        head = {"f": [s["xI"], s["xJ"], s["start"], s["wh"], np_], "e": [s["xI"], s["xJ"], s["bI"], s["bJ"], s["start"], s["wh"], s["K"], np_],
                "ea": [s["bI"], s["bJ"], s["start"], np_, upright], "eo": [s["xI"], s["xJ"], s["start"], s["wh"], s["bound"], np_]}
    functor = geofilter.GeometricFilter_FMatrix_AC(PRECISION[model], ITERATIONS)
    mask, res, st = geofilter._run(_ENTRY[model] + ("_indexed" if indexed else ""), -1, head[{"h": "f", "eu": "ea"}.get(model, model)], s["n_matches"], np_, functor)
    return mask.tobytes(), res.tobytes(), int(st.n_iterations), int(st.n_models), res


@contextlib.contextmanager
def _environment(**values):
    """the launch-form switches of the library for the calls inside the block; the others unset; restored on the way out"""
    names = ("MVGX_GEO_GLOBAL_ABOVE", "MVGX_GEO_AHEAD", "MVGX_GEO_E_AHEAD")
    saved = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def output(model, limit, emulated, indexed=False, **env):
    """call() on the model's scene under the emulation or on the device, computed once per form"""
    with _environment(**env), (_emu.emulated() if emulated else contextlib.nullcontext()):
        return call(scene(model, limit), indexed)


def check_indexed_equals_gathered(model, limit, emulated):
    g, x = output(model, limit, emulated), output(model, limit, emulated, indexed=True)
    assert g[2] > len(sizes(model, limit)) - 2 and g[3] >= g[2], g[2:4]   # (every pair of more than m correspondences ran)
    assert x[2:4] == g[2:4] and x[0] == g[0] and x[1] == g[1]


def check_global_form_equals_default(model, limit, emulated):
    g, t = output(model, limit, emulated), output(model, limit, emulated, MVGX_GEO_GLOBAL_ABOVE="8")
    assert t[2:4] == g[2:4] and t[0] == g[0] and t[1] == g[1]


def check_one_sample_per_iteration_equals_default(model, limit, emulated):
    assert model in ("h", "e")   # the models with a samples-ahead instantiation
    g, one = output(model, limit, emulated), output(model, limit, emulated, MVGX_GEO_AHEAD="1")
    assert one[2:4] == g[2:4] and one[0] == g[0] and one[1] == g[1]


def check_small_pairs_are_rejected(model, limit, emulated):
    s = scene(model, limit)
    n = np.diff(s["start"].astype(np.int64))
    for form in (output(model, limit, emulated), output(model, limit, emulated, indexed=True)):
        res, mask = form[4], np.frombuffer(form[0], bool)
        small = np.flatnonzero(n <= MIN_SAMPLE[model])
        assert len(small) == 2
        for p in small:
            assert not res["ok"][p] and res["n_inliers"][p] == 0 and np.array_equal(res["F"][p], np.eye(3)), (model, p)
            assert not mask[int(s["start"][p]):int(s["start"][p + 1])].any()
