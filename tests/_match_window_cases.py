"""Inputs and checks of the window structure of the default matching filter (l2_filter16_kernel): a database image streams
through windows of 8 tiles; a full window runs unrolled with its first tile peeled (the first epilogue of every window maximum WRITES it),
the one short window of an image keeps a tile loop; the window maxima are folded into a running top-2 once per window. Shared by the GPU
test and by the CPU test that runs the same device source under the HIP emulation.

Database images. All rows of an image get the same norm parity (tests._match_wave_cases.force_norm_parity), so the rows fill only one half
of every tile, in their order: row r is slot r % 16 of tile r // 16, and the image has exactly ceil(n / 16) tiles:

    n       16    112    128       129         256        257
    tiles   1     7      8         9           16         17
    windows short short  full      full + 1    full full  full full + 1

and one image of 300 rows of natural parity. Where a row falls decides which path of the kernel sees it, so near-duplicates are PLANTED:
a query q = b + small noise of a chosen "best" row b, and a runner-up row u = b + noise that decides the ratio test. The best rows sit in

    first   the first tile of a window (the peeled one)            last    the last tile of a full window
    second  the first tile of the second window                    single  the only tile (one row) of a one-tile last window
            (256 and 257 rows)                                             (129 and 257 rows; row 128 of 129 is both, listed here)

and the runner-up, relative to the best row's cell (P-class, lane group, window: the 16 rows the filter does not tell apart),

    cell    in the same cell (slot j ^ 1 of the same tile): the filter passes a candidate and the verify stage decides
    class   in another P-class of the same window (slot j ^ 2)      window  in another window

each with a far runner-up (the reference accepts the match) and a near one (it rejects). What the reference does with every planted
query is asserted from its lists alone (check_cases_are_what_they_claim), so the inputs cannot drift away from the cases."""
import functools

import numpy as np

from openmvg_amd import matching
from tests import _oracle
from tests._match_wave_cases import force_norm_parity, tiles

RATIO = 0.8
FORCED = [16, 112, 128, 129, 256, 257]          # rows of the database images of one norm parity
TILES = [1, 7, 8, 9, 16, 17]
NATURAL = 300                                    # ... and of the one of natural parity
QUERY_ROWS = [1, 33, 129]
BATCH_PAIRS = 11                                 # 21 pairs: two batches


def _places(n):
    """{place: first row of its tile} of a database image of n rows of one parity"""
    nt = -(-n // 16)
    out = {"first": 0}
    if nt >= 8:
        out["last"] = 7 * 16
    if nt > 8:
        out["second"] = 8 * 16
    if nt > 8 and nt % 8 == 1:
        out["single"] = (nt - 1) * 16
    return out


def _plan(n):
    """[(place, kind, accept, best row, runner-up row)]: every combination the image has room for, no row used twice"""
    places = _places(n)
    used, plan = set(), []

    def other_window(b):   # a free row of another window, outside the quads of a tile that hold best rows
        return next((r for r in range(n) if r // 128 != b // 128 and r % 16 >= 12 and r not in used), None)

    for place, t0 in places.items():
        if place == "single":   # one row: the best row of one accepted query, its runner-up in another window
            combos = [("window", True, 0)]
        else:
            combos = [("cell", True, 0), ("cell", False, 2), ("class", True, 4), ("class", False, 5), ("window", True, 8), ("window", False, 9)]
        for kind, accept, j in combos:
            b = t0 + j
            u = b ^ 1 if kind == "cell" else b ^ 2 if kind == "class" else other_window(b)
            if b >= n or b in used or u is None or u >= n or u in used:
                continue
            used.update((b, u))
            plan.append((place, kind, accept, b, u))
    return plan


def _plant(rng, d, plan):
    """writes the runner-ups into the database image d and returns the planted queries, one per plan entry"""
    q = np.empty((len(plan), 128), np.int16)
    for k, (_, _, accept, b, u) in enumerate(plan):
        d[b] = rng.integers(48, 208, 128)                  # no clipping below
        e0 = rng.integers(-2, 3, 128)
        q[k] = d[b].astype(np.int16) + e0                  # d0 = |e0|^2, about 256
        if accept:
            d[u] = d[b].astype(np.int16) + rng.integers(-12, 13, 128)       # d1 about 6 600: d0 < 0.64 d1
        else:
            e2 = np.zeros(128, np.int16); e2[rng.choice(128, 6, replace=False)] = 1
            d[u] = d[b].astype(np.int16) + 2 * e0 + e2     # d1 = |e0 + e2|^2 within 6 + 2 * 12 of d0: d0 >= 0.64 d1
    return q


@functools.lru_cache(maxsize=None)
def images():
    """(images, pairs, plants): database image k, then its three query images; plants[(db index, query index)] = [(query row, best row,
    place, kind, accept)]"""
    rng = np.random.default_rng(2025)
    imgs, pairs, plants = [], [], {}
    for n in FORCED + [NATURAL]:
        d = rng.integers(0, 256, (n, 128)).astype(np.uint8)
        if n == NATURAL:   # natural parity: the rows' slots follow their parities, so the plants are plain near-duplicates of neighbours
            plan = [("any", "any", k % 2 == 0, 20 * k + 3, 20 * k + 4) for k in range(12)]
        else:
            plan = _plan(n)
        q = _plant(rng, d, plan)
        if n != NATURAL:
            d = force_norm_parity(d, n & 1)                 # (after planting; one LSB of byte 0: far inside every margin above)
        q = np.clip(q, 0, 255).astype(np.uint8)
        di = len(imgs)
        imgs.append(d)
        for m in QUERY_ROWS:
            # the planted queries first (as many as fit; the 129-row image takes them in reverse), then noisy copies of other rows
            order = list(range(len(plan)))
            if m == 129:
                order.reverse()
            order = order[:m]
            rest = rng.integers(0, n, m - len(order))
            fill = np.clip(d[rest].astype(np.int16) + rng.integers(-6, 7, (len(rest), 128)), 0, 255).astype(np.uint8)
            qi = len(imgs)
            imgs.append(np.ascontiguousarray(np.concatenate([q[order], fill]) if len(order) else fill))
            pairs.append((di, qi))
            plants[(di, qi)] = [(row, plan[k][3], plan[k][0], plan[k][1], plan[k][2]) for row, k in enumerate(order)]
    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs), np.ascontiguousarray(np.array(pairs, np.uint32)), plants


@functools.lru_cache(maxsize=None)
def reference():
    """{(I, J): (n, 2) array of (row of I, row of J)} from the compiled reference; from its C restatement where oracle/_ref is absent"""
    imgs, pairs, _ = images()
    if _oracle.have_ref_match():
        ref = _oracle.ref_matcher_regions_match(list(imgs), pairs, RATIO)
    else:
        off, ij = _oracle.port_matcher_regions_match(list(imgs), pairs, RATIO)
        ref = _oracle.offsets_to_dict(pairs, off, ij)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def check_cases_are_what_they_claim():
    imgs, pairs, plants = images()
    ref = reference()
    dbs = sorted({int(i) for i, _ in pairs})
    assert [tiles(imgs[i]) for i in dbs[:-1]] == TILES and [len(imgs[i]) for i in dbs] == FORCED + [NATURAL]
    odd = int((((imgs[dbs[-1]].astype(np.int64) - 128) ** 2).sum(axis=1) & 1).sum())
    assert tiles(imgs[dbs[-1]]) > 8 and 100 < odd < 200          # two windows, both parities
    want_places = [{"first"}, {"first"}, {"first", "last"}, {"first", "last", "single"}, {"first", "last", "second"},
                   {"first", "last", "second", "single"}]
    seen_kinds = set()
    for di, want in zip(dbs, want_places + [{"any"}]):
        verdicts, got_places = set(), set()
        for (i, j), pl in plants.items():
            if i != di:
                continue
            m = ref.get((i, j), np.zeros((0, 2), np.uint32))
            by_query = {int(b): int(a) for a, b in m}
            for row, best, place, kind, accept in pl:
                # the reference does with every planted query what the plan says: accepts it with the planted best row, or rejects it
                assert (by_query.get(row) == best) if accept else (row not in by_query), (di, j, row, best, place, kind, accept)
                verdicts.add(accept); got_places.add(place)
                if len(imgs[j]) >= 33:
                    seen_kinds.add((kind, accept))
        assert verdicts == {True, False}, di          # queries on both sides of the ratio test
        assert got_places == want, (di, got_places)
    assert seen_kinds >= {(k, a) for k in ("cell", "class", "window") for a in (True, False)}
    assert sum(len(v) for v in ref.values()) > 500    # equality with it is not vacuous
    assert len(pairs) > BATCH_PAIRS


def _assert_lists(pairs, off, ij):
    ref = reference()
    got = _oracle.offsets_to_dict(pairs, off, ij)
    for k in {tuple(map(int, p)) for p in pairs}:
        want = ref.get(k, np.zeros((0, 2), np.uint32))
        have = got.get(k, np.zeros((0, 2), np.uint32))
        assert np.array_equal(np.asarray(have).reshape(-1, 2), np.asarray(want).reshape(-1, 2)), (k, have[:5], want[:5])


def check_lists():
    """the default form, two batches; then a parity-slot filter (32x32x32) on the SAME context - it leaves its own codes in best[] and walks
    the other work list - and the default form again: every run's lists equal the reference's, entry by entry"""
    imgs, pairs, _ = images()
    r2 = np.float32(RATIO) * np.float32(RATIO)
    ctx = matching.MatchContext(0)
    try:
        ctx.set_option("variant", 4); ctx.set_option("stage", 3); ctx.set_option("filter_shape", 16)
        ctx.set_option("batch_pairs", BATCH_PAIRS)
        ctx.set_regions(list(imgs))
        for shape in (16, 32, 16):
            ctx.set_option("filter_shape", shape)
            _, off, ij = ctx.run(pairs, r2)          # (raises when the verify stage disagrees with the filter's best distance)
            _assert_lists(pairs, off, ij)
    finally:
        ctx.close()
