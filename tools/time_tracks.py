"""Times mvgx_tracks_build on the MI355X on synthetic match graphs: 1 000 images x 2 000 features with the track lengths of
synth.geometric_track_lengths, then the same points with every pair of a point's images matched (5.0 x the matches: all the pairs
there are; the 10 x budget is not reached at this length distribution), 5 % of the matches wrong.

  python tools/time_tracks.py [--images 1000] [--features 2000] [--repeat 5] [--wrong 0.05] [--dump DIR]

Prints one JSON line per size: medians over --repeat calls after one warm-up call of the device time of every pass (HIP events around its
launches), kernel_ms (their sum), total_ms (the whole call with uploads, downloads and the host's waits) and n_sweeps; beside them the
bytes every pass reads and writes by the arithmetic of its arrays (no cache counted) and that traffic over the pass's time as a fraction
of 8 TB/s. --dump DIR writes pairs.npy / match_start.npy / ij.npy of every size into DIR/<size>/ - the inputs
`python tests/golden/make_tracks_golden.py --time DIR/<size>` hands to the compiled reference on the machine that has its tree.
Needs a GPU: there is no CPU path.

The graph: a point is seen by `length` images chosen at random; size 1: the images of a point are matched along a chain (image k with
image k + 1 of the point, length - 1 matches); size 10 (the label kept from the budget): every image of a point with every later one,
cut at 10 x the chain's matches - 5.0 x are reached."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openmvg_amd import _capi, synth, tracks   # noqa: E402

PASSES = ("extent", "mark", "number", "label", "collide", "select", "gather", "replay", "export")
HBM_BYTES_PER_MS = 8.0e9   # 8 TB/s


def match_graph(n_images, n_features, dense, wrong, seed=0x7AC7):
    rng = np.random.default_rng(seed)
    n_points = n_images * n_features // 6
    length = np.minimum(synth.geometric_track_lengths(n_points, mean=6.0, lo=2, hi=40, seed=seed), n_images)
    point = np.repeat(np.arange(n_points), length)
    # distinct images of a point: a random start, then random steps whose sum stays below n_images; ascending inside the point
    assert n_images >= 100, "the image draw needs 100 images or more"
    hi = int(length.max())
    walk = (rng.integers(0, n_images, (n_points, 1)) + np.cumsum(rng.integers(1, n_images // (hi + 1) + 1, (n_points, hi)), axis=1)) % n_images
    walk[np.arange(hi)[None, :] >= length[:, None]] = n_images   # (beyond the point's length: sorted to the end, dropped)
    walk = np.sort(walk, axis=1)
    image = walk[walk < n_images]
    # the feature index of an observation: its position among the observations of its image
    order = np.argsort(image, kind="stable")
    first = np.concatenate([[0], np.cumsum(np.bincount(image, minlength=n_images))])
    feature = np.empty(len(image), np.int64)
    feature[order] = np.arange(len(image)) - first[image[order]]
    start = np.concatenate([[0], np.cumsum(length)])
    within = np.arange(len(image)) - start[point]
    a, b = [], []
    chain = np.flatnonzero(within + 1 < length[point])
    budget = 10 * len(chain)
    for step in range(1, int(length.max()) if dense else 2):
        src = np.flatnonzero(within + step < length[point])
        a.append(src); b.append(src + step)
        if sum(len(v) for v in a) >= budget:
            break
    a, b = np.concatenate(a)[:budget if dense else None], np.concatenate(b)[:budget if dense else None]
    fi, fj = feature[a].copy(), feature[b].copy()
    bad = np.flatnonzero(rng.random(len(a)) < wrong)
    fj[bad] = rng.integers(0, np.bincount(image, minlength=n_images)[image[b[bad]]])
    key = image[a] * n_images + image[b]
    by_pair = np.argsort(key, kind="stable")
    pairs_key, counts = np.unique(key, return_counts=True)
    pairs = np.stack([pairs_key // n_images, pairs_key % n_images], axis=1).astype(np.uint32)
    match_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    ij = np.stack([fi[by_pair], fj[by_pair]], axis=1).astype(np.uint32)
    return pairs, match_start, ij, np.bincount(image, minlength=n_images).astype(np.uint32)


def pass_bytes(st, n_pairs, n_keys):
    """bytes read + written per pass, by the arrays each kernel walks (4-byte entries unless said; a binary search over match_start counted
    as log2 reads of 8 bytes; scattered 4-byte accesses counted as 4 bytes; gather and replay as if every kept match belonged to a
    survivor: an upper figure where many matches sit in dropped components)"""
    m, n, t, o = int(st.n_matches_used), int(st.n_nodes), int(st.n_tracks), int(st.n_obs)
    scan = lambda k: 4 * (3 * k + 1)   # noqa: E731  (read for the sums, read and write for the scan)
    return dict(mark=m * (8 + 8 * np.log2(max(n_pairs, 2)) + 8 + 16 + 8 + 8), number=scan(n_keys) + 8 * n_keys + 8 * n + 16 * m + 12 * n,
                label=int(st.n_sweeps) * (m * (8 + 32) + n * (16 + 4)), collide=n * (4 + 16), select=n * (4 + 8) + n * 16 + scan(n) + 12 * n,
                gather=2 * m * 16 + scan(n) + 4 * m, replay=t * 16 + 3 * 4 * m + 16 * m, export=2 * scan(n) + 12 * n + 8 * t + scan(t) + 24 * n + 4 * o + 8 * o * 3 + 8 * o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--wrong", type=float, default=0.05)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("time_tracks.py needs a GPU")
    debug = _capi.lib().mvgx_debug_tracks_pass_ms   # a measuring aid outside include/mvgx.h
    debug.restype, debug.argtypes = C.c_int, [C.POINTER(C.c_double), C.c_int]
    for size, dense in ((1, False), (10, True)):
        pairs, match_start, ij, n_features = match_graph(a.images, a.features, dense, a.wrong)
        if a.dump:
            d = os.path.join(a.dump, str(size))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "pairs.npy"), pairs); np.save(os.path.join(d, "match_start.npy"), match_start); np.save(os.path.join(d, "ij.npy"), ij)
        rows = []
        for r in range(a.repeat + 1):
            t = tracks.build(pairs, match_start, ij, n_images=a.images, n_features=n_features)
            ms = (C.c_double * len(PASSES))()
            _capi.check(debug(ms, len(PASSES)))
            if r:   # (the first call warms up: code objects, the stream)
                rows.append(dict(zip(PASSES, ms), kernel_ms=t.stats.kernel_ms, total_ms=t.stats.total_ms, n_sweeps=int(t.stats.n_sweeps)))
        med = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
        st = t.stats
        traffic = pass_bytes(st, len(pairs), int(n_features.sum()))
        print(json.dumps(dict(size=size, images=a.images, pairs=len(pairs), matches=len(ij), nodes=int(st.n_nodes), components=int(st.n_components),
                              collisions=int(st.n_collision), tracks=int(st.n_tracks), observations=int(st.n_obs), **{k: round(v, 4) for k, v in med.items()},
                              bytes={k: int(v) for k, v in traffic.items()},
                              hbm_fraction={k: round(float(v) / max(med[k], 1e-9) / HBM_BYTES_PER_MS, 4) for k, v in traffic.items()})), flush=True)


if __name__ == "__main__":
    main()
