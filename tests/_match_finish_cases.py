"""Inputs and checks of the transposed finish of the default matching filter (l2_filter16_kernel, DESIGN.md 3.3 "The finish, transposed"):
after the last window the four lane groups of a wave exchange halves of their eight (W1, V2, code) triples, so that lane group g merges
and stores blocks own0(g) and own0(g) + 1 of the wave's unit, own0 = 4 (g & 1) + 2 (g >> 1). Shared by the GPU test and by the CPU test
that runs the same device source under the HIP emulation (there the exchange is its shuffle-and-select form: the ownership, the operand
roles of the merge and the store addressing are the same code).

What can go wrong is a property of WHERE things sit: the block of the unit a query row is in (who owns it), the lane group that holds the
best database row and the one that holds the runner-up (which operand of which merge they are). The inputs are built so that the
reference's own lists cover every combination; inputs_cover_the_finish_cases() restates the slot rule (a row's rank within its norm
parity, slot_row) on the host and asserts it. Results are integers and are compared for equality with
_oracle.port_matcher_regions_match; every run relies on the context's error flag as tests/_match_wave_cases.py explains."""
import functools

import numpy as np

from openmvg_amd import matching
from tests import _oracle

RATIO = 0.8
R2 = np.float32(RATIO) * np.float32(RATIO)

# Three database images (0..2) and four runs of query images, every query image in one run. Blocks of 16 rows per query image, in run order:
#   run of 0:  9 10 11 12 13 14 15 4 1   the units split at 1, 3, 6, 2, 7, 5, 4 (every point) and the run ends in a unit of ONE block
#   run of 1:  3 2 6 7 5 1               last blocks of 1, 15 and 16 rows under the owners the first run leaves out
#   run of 2:  1                         one block of one row: blocks 1..7 of its unit are past nJ, the second segment is absent
#   run of 1:  7                         (once more) a last block of 15 rows under lane group 3
DB = [250, 200, 129]
RUNS = [
    (0, [129, 160, 175, 192, 193, 224, 239, 64, 16]),
    (1, [33, 31, 96, 97, 79, 1]),
    (2, [1]),
    (1, [111]),
]
SIZES = DB + [n for _, js in RUNS for n in js]
OWNER_OF_BLOCK = [0, 0, 2, 2, 1, 1, 3, 3]   # lane group that finishes block n of a unit


def blocks(n):
    return -(-n // 16)


@functools.lru_cache(maxsize=None)
def pair_list():
    out, j = [], len(DB)
    for I, js in RUNS:
        for _ in js:
            out.append((I, j))
            j += 1
    return np.ascontiguousarray(np.array(out, np.uint32))


def units_of(pairs, batch_pairs=None):
    """the partition DESIGN.md 3.2 describes (as tests/_match_block_cases.py restates it): a list of units, each a list of segments
    (pair, J, first block, blocks), closed at 8 blocks, at a change of I, at the end of a batch and before a third image"""
    pairs = np.asarray(pairs)
    step = batch_pairs or len(pairs)
    out = []
    for k0 in range(0, len(pairs), step):
        unit, unit_I = None, None
        for k in range(k0, min(k0 + step, len(pairs))):
            I, J = int(pairs[k][0]), int(pairs[k][1])
            if SIZES[I] < 2 or SIZES[J] == 0:
                continue
            blk, nblk = 0, blocks(SIZES[J])
            while blk < nblk:
                if unit is None or unit_I != I or sum(s[3] for s in unit) == 8 or len(unit) == 2:
                    unit, unit_I = [], I
                    out.append(unit)
                take = min(nblk - blk, 8 - sum(s[3] for s in unit))
                unit.append((k, J, blk, take))
                blk += take
    return out


def block_in_unit(units):
    """(pair, block of J) -> block 0..7 of its unit"""
    out = {}
    for u in units:
        at = 0
        for k, _, b0, nb in u:
            for b in range(nb):
                out[(k, b0 + b)] = at + b
            at += nb
    return out


def lane_groups(img):
    """lane group 0..3 of l2_filter16_kernel that sees each row of a database image: rows are dealt to slots in rank order within their
    norm parity; rank r of parity h sits in in-tile row slot_row(r & 15, h) = ((r & 15) >> 2) * 8 + 4 h + (r & 3), row m of a tile is row
    m & 15 of a 16-row block, and the MFMA hands rows 4 g .. 4 g + 3 of a block to lane group g"""
    c = img.astype(np.int64) - 128
    par = ((c * c).sum(axis=1) & 1).astype(np.int64)
    rank = np.zeros(len(img), np.int64)
    for h in (0, 1):
        rank[par == h] = np.arange(int((par == h).sum()))
    m = ((rank & 15) >> 2) * 8 + 4 * par + (rank & 3)
    return (m & 15) >> 2


def _near(rng, row, amp=9):
    return np.clip(row.astype(np.int16) + rng.integers(-amp, amp + 1, row.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def images():
    """database images of uniform bytes; a query image holds, row by row, a near-duplicate of a random database row (an accepted match
    whose winner and runner-up fall in random lane groups), a blend of two database rows of different lane groups near the ratio
    threshold (both sides of the test), or noise. In the first run one row under each owning lane group is a near-duplicate of a
    database row that exists TWICE, in lane groups g and g ^ 2: a tie for the first place (see ties())."""
    rng = np.random.default_rng(20251)
    imgs = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in SIZES]
    # two database rows of image 0 duplicated into the lane group across (same norm, hence same parity and unchanged ranks)
    g0 = lane_groups(imgs[0])
    dup = []
    for g in (0, 1):
        a = int(np.flatnonzero(g0 == g)[3]); b = int(np.flatnonzero(g0 == (g ^ 2))[5])
        imgs[0][b] = imgs[0][a]
        dup.append((a, b))
    assert np.array_equal(lane_groups(imgs[0]), g0)
    for k, (I, J) in enumerate(pair_list()):
        D, Q = imgs[int(I)], imgs[int(J)]
        gD = lane_groups(D)
        for q in range(len(Q)):
            kind = rng.integers(0, 10)
            if kind < 6:
                Q[q] = _near(rng, D[rng.integers(0, len(D))])
            elif kind < 8 and len(D) > 4:
                a = int(rng.integers(0, len(D))); b = int(rng.choice(np.flatnonzero(gD != gD[a])))
                t = rng.uniform(0.40, 0.49)    # d0 / d1 = (t / (1 - t))^2: 0.44 .. 0.92 around 0.64
                Q[q] = np.clip(np.rint(D[a] + t * (D[b].astype(np.float64) - D[a])), 0, 255).astype(np.uint8)
    # the ties: pair k of the first run, row q of a block under each owner, for both duplicated rows
    where = block_in_unit(units_of(pair_list()))
    placed = []
    for owner in range(4):
        for which, (a, b) in enumerate(dup):
            k, blk = next((k, blk) for (k, blk), n in sorted(where.items())
                          if pair_list()[k][0] == 0 and OWNER_OF_BLOCK[n] == owner and n % 2 == which
                          and 16 * blk + 16 <= SIZES[int(pair_list()[k][1])])
            J = int(pair_list()[k][1])
            q = 16 * blk + 3 + 2 * which
            imgs[J][q] = _near(rng, imgs[0][a], 2)
            placed.append((k, q, a, b))
    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs), tuple(placed)


def ties():
    return images()[1]


@functools.lru_cache(maxsize=None)
def reference():
    off, ij = _oracle.port_matcher_regions_match(list(images()[0]), pair_list(), RATIO)
    off.setflags(write=False); ij.setflags(write=False)
    return off, ij


@functools.lru_cache(maxsize=None)
def nearest_two():
    """per pair: (best row, runner-up row, d0, d1) of every query row, by brute force on the host (first index wins a tie, as in the
    reference)"""
    imgs = images()[0]
    out = []
    for I, J in pair_list():
        D = imgs[int(I)].astype(np.int64); Q = imgs[int(J)].astype(np.int64)
        d = (Q * Q).sum(1)[:, None] + (D * D).sum(1)[None, :] - 2 * Q @ D.T
        order = np.argsort(d, axis=1, kind="stable")[:, :2]
        out.append((order[:, 0], order[:, 1], np.take_along_axis(d, order[:, :1], 1)[:, 0], np.take_along_axis(d, order[:, 1:2], 1)[:, 0]))
    return out


def inputs_cover_the_finish_cases():
    """the inputs cannot drift away from the cases: asserted on the reference's lists and the slot rule alone"""
    pairs = pair_list()
    imgs = images()[0]
    assert max(SIZES) <= 250
    units = units_of(pairs)
    where = block_in_unit(units)
    # unit splits at every point, the two blocks one lane group owns in different pairs (odd splits), an absent second segment
    two = [u for u in units if len(u) == 2]
    assert {u[0][3] for u in two} == set(range(1, 8))
    assert any(len(u) == 1 and u[0][3] == 1 for u in units)
    # last blocks of 1, 15 and 16 rows under every owner
    last = {(OWNER_OF_BLOCK[where[(k, blocks(SIZES[J]) - 1)]], (SIZES[J] - 1) % 16 + 1) for k, (I, J) in enumerate(pairs)}
    assert {(o, r) for o in range(4) for r in (1, 15, 16)} <= last, sorted(last)
    # blocks wholly past nJ under every owner: the blocks of a unit behind its last segment
    past = {OWNER_OF_BLOCK[n] for u in units for n in range(sum(s[3] for s in u), 8)}
    assert past == {0, 1, 2, 3}
    # the accepted matches of the reference: (block of the unit, winner's lane group) and (winner's group, runner-up's group)
    off, ij = reference()
    assert int(off[-1]) > 800
    near = nearest_two()
    blk_grp, win_run, rej_cross_near, acc_cross_near = set(), set(), 0, 0
    for k, (I, J) in enumerate(pairs):
        g = lane_groups(imgs[int(I)])
        i1, i2, d0, d1 = near[k]
        acc = np.zeros(SIZES[int(J)], bool)
        m = ij[int(off[k]):int(off[k + 1])]
        acc[m[:, 1]] = True
        assert np.array_equal(i1[m[:, 1]], m[:, 0])          # (the host's nearest row is the reference's)
        if len(g) < 2:
            continue
        for q in range(SIZES[int(J)]):
            cross = g[i1[q]] != g[i2[q]]
            close = d0[q] < d1[q] and 0.4 * d1[q] < d0[q] < 0.95 * d1[q]      # the ratio test decides, not a tie
            if acc[q]:
                blk_grp.add((where[(k, q >> 4)], int(g[i1[q]])))
                win_run.add((int(g[i1[q]]), int(g[i2[q]])))
                acc_cross_near += bool(cross and close)
            else:
                rej_cross_near += bool(cross and close)
    assert blk_grp == {(n, gg) for n in range(8) for gg in range(4)}, sorted(blk_grp)
    assert win_run == {(a, b) for a in range(4) for b in range(4)}, sorted(win_run)
    assert acc_cross_near > 20 and rej_cross_near > 20, (acc_cross_near, rej_cross_near)   # both sides of the ratio test, runner-up elsewhere
    # the ties: equal best rows in lane groups g and g ^ 2, one query under each owner for both g; the reference rejects them
    g0 = lane_groups(imgs[0])
    seen = set()
    for k, q, a, b in ties():
        i1, i2, d0, d1 = near[k]
        assert pairs[k][0] == 0 and {int(i1[q]), int(i2[q])} == {a, b} and d0[q] == d1[q]
        assert g0[a] == g0[b] ^ 2
        m = ij[int(off[k]):int(off[k + 1])]
        assert q not in m[:, 1]
        seen.add((OWNER_OF_BLOCK[where[(k, q >> 4)]], int(g0[a]) & 1))
    assert seen == {(o, h) for o in range(4) for h in (0, 1)}, sorted(seen)
    # two batches and more at the batch size check_reused_slots() uses
    assert len(pairs) > 3 * 5 and units_of(pairs, 5) != units   # (batch ends cut units inside a run: other blocks meet other owners)
    return units


def context(batch_pairs=None):
    """the default kernel (variant 4, every stage, the 16x16x64 filter)"""
    ctx = matching.MatchContext(0)
    ctx.set_option("variant", 4); ctx.set_option("stage", 3); ctx.set_option("filter_shape", 16)
    if batch_pairs:
        ctx.set_option("batch_pairs", batch_pairs)
    ctx.set_regions(list(images()[0]))
    return ctx


def check_lists():
    """offsets and (i, j) lists of the whole pair list, entry by entry"""
    want_off, want_ij = reference()
    ctx = context()
    try:
        _, off, ij = ctx.run(pair_list(), R2)     # (raises when the error flag is not zero)
    finally:
        ctx.close()
    assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij)


def check_reused_slots():
    """batches of 5 pairs on one context, with a run of the 32x32x32 filter in between: that filter numbers best[] by parity slot and
    leaves its own codes there, and every batch slot is written again by other units' owners"""
    want_off, want_ij = reference()
    ctx = context(5)
    try:
        for shape in (16, 32, 16):
            ctx.set_option("filter_shape", shape)
            _, off, ij = ctx.run(pair_list(), R2)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), shape
    finally:
        ctx.close()
