"""Inputs and checks of the verify stage that runs after the default matching filter (l2_verify_kernel<true>): a wave
takes the candidates the filter left in the 128 query slots of its unit (two parts of 64 slots, up to two pairs), ranks them over both
parts and hands candidate 4 k + sub of the unit to lane group `sub` in round k. 16 lanes recompute the 16 rows of the winner's cell, with
the norms read from the per-slot tables. Shared by the GPU test and by the CPU test that runs the same device source under the HIP
emulation.

What decides which path of the kernel a query takes is (a) how many candidates its part and its unit hold and in which lanes, (b) the
shape of the database image, which says how many slots of the winner's cell are pad slots, and (c) where the runner-up lies. A random
query is no candidate (its two nearest rows are about equally far), a near-duplicate of a database row is one: so candidates are PLANTED.

Database images (index: rows): natural norm parity with 1, 15, 16, 17, 40 and 530 rows (530: three windows, the window field of the
code word takes 0, 1 and 2), and SKEW, 40 rows of which the first 37 have an even and the last 3 an odd squared norm: its rows sit in
slot rank % 16 of tile rank // 16 of their half, the odd half's only tile holds 13 pad slots.

Query images.
  COUNTS (against the 530-row image) is a sequence of whole units of 128 rows; UNITS says which lanes of part 0 and of part 1 of each
    hold a candidate: none, 1, 4 (lanes 0, 15, 16, 63), 5, 7 + 6 (two parts joined in one round), 64 + 0, 0 + 64, 64 + 64 (ranks past
    63), 60 + 9 (part 1's ranks wrap) and 0 + 2. Every fifth candidate of a part is one the verify stage REJECTS: a second database row
    of the winner's cell is as close as the winner. The others are accepted.
  HEAD, TAIL, MID and LAST (40, 150, 80 and 50 rows against the 530-row image, after COUNTS): units that hold the last blocks of one pair
    and the first of the next - 3 + 5 blocks (split inside part 0), 5 + 3 (inside part 1) and 2 + 4. Both segments hold candidates.
  One query image per small database image: near-duplicates of its rows and random rows.
  CELL against SKEW: the runner-up inside the winner's cell, at exact distances (steps of 2 keep a row's norm parity; D0 = 64):
    near        same tile, winner at an even slot;  d1 = 98: rejected (the filter saw no row of the cell but the winner: it let it pass)
    accept      same tile, winner at an odd slot;   d1 = 100: accepted by the fp32 test alone - 64 < 0.64 * 100 is false, but the
                float32 square of 0.8f lies above 0.64 and float32(r2 * 100.f) is the float after 64.f
    near2/acc2  the same two with the runner-up in the next tile of the cell
    tie/tie2    the runner-up equals the winner (same tile / next tile): d0 = d1, the reference rejects
    odd         winners in the odd half: 13 of the 16 slots of the cell's only occupied tile are pad slots
  What the reference does with each is asserted from its lists (inputs_are_what_they_claim).

Lists are integers and are compared entry by entry with the compiled reference (oracle/_ref, through tests/_oracle; its C restatement
where that is not built). Every run also requires the context's error flag to be zero: MatchContext.run raises when the verify stage
finds a winner that differs from the filter's (dbest != f_d0) or a cell without a valid row."""
import functools

import numpy as np

from openmvg_amd import matching
from tests import _oracle

RATIO = 0.8
R2 = np.float32(RATIO) * np.float32(RATIO)
DB_ROWS = [1, 15, 16, 17, 40, 530]
BIG = DB_ROWS.index(530)
SKEW = len(DB_ROWS)                       # 40 rows: 37 even, 3 odd
SKEW_EVEN = 37
ALL64 = tuple(range(64))
UNITS = [((), ()), ((0,), ()), ((0, 15, 16, 63), ()), ((3, 15, 16, 40, 63), ()), ((1, 2, 17, 30, 31, 47, 62), (0, 5, 16, 33, 48, 63)),
         (ALL64, ()), ((), ALL64), (ALL64, ALL64), (tuple(range(2, 62)), (0, 7, 8, 15, 16, 31, 32, 47, 63)), ((), (0, 63))]
SPLIT_ROWS = {"HEAD": 40, "TAIL": 150, "MID": 80, "LAST": 50}
D0 = 64                                   # the planted exact cases: 16 steps of 2


def _odd(d):
    return (((d.astype(np.int64) - 128) ** 2).sum(axis=1) & 1).astype(bool)


def _near(rng, row, amp=2):
    return np.clip(row.astype(np.int16) + rng.integers(-amp, amp + 1, 128), 0, 255).astype(np.uint8)


def _steps(rng, row, n_two, n_one=0, avoid=()):
    """row + 2 on n_two coordinates and + 1 on n_one others (an even number keeps the norm parity), none of them in `avoid`"""
    free = np.setdiff1d(np.arange(128), np.asarray(avoid, np.int64))
    pick = rng.choice(free, n_two + n_one, replace=False)
    out = row.astype(np.int16)
    out[pick[:n_two]] += 2
    out[pick[n_two:]] += 1
    return out.astype(np.uint8), pick


@functools.lru_cache(maxsize=None)
def images():
    """(images, pairs, plan): plan[(I, J)] = {query row: (accept, best row of I or None)} for every planted query"""
    rng = np.random.default_rng(77)
    dbs = [rng.integers(48, 208, (n, 128)).astype(np.uint8) for n in DB_ROWS]
    skew = rng.integers(48, 208, (40, 128)).astype(np.uint8)
    flip = _odd(skew) != (np.arange(40) >= SKEW_EVEN)
    skew[flip, 0] ^= 1
    imgs, pairs, plan = dbs + [skew], [], {}

    # --- the 530-row image: reject plants. Row u of rank k ^ 1 of the same half (same tile, same cell) becomes b + steps of 2: the rows keep
    # their parities, so every rank stays what it was
    big = imgs[BIG]
    odd = _odd(big)
    rank = np.where(odd, np.cumsum(odd) - 1, np.cumsum(~odd) - 1)
    by_rank = {(bool(o), int(k)): r for r, (o, k) in enumerate(zip(odd, rank))}
    rej = []
    for b in range(7, 530, 23):                      # 23 rows spread over the image: every window
        u = by_rank.get((bool(odd[b]), int(rank[b]) ^ 1))
        if u is not None:
            big[u], _ = _steps(rng, big[b], 3)
            rej.append((b, u))
    taken = {r for bu in rej for r in bu}
    assert len(taken) == 2 * len(rej) and np.array_equal(_odd(big), odd)
    acc = [r for r in range(530) if r not in taken]

    def fill_big(n_rows, lanes_of_row):
        """a query image against the 530-row image: random rows, a plant where lanes_of_row says so (every fifth one a reject)"""
        q = rng.integers(0, 256, (n_rows, 128)).astype(np.uint8)
        pl, seen = {}, 0
        for row in range(n_rows):
            if not lanes_of_row(row):
                continue
            seen += 1
            if seen % 5 == 0:
                b = rej[(seen // 5) % len(rej)][0]
                pl[row] = (False, None)
            else:
                b = acc[(seen * 37) % len(acc)] if seen % 3 else acc[-1 - (seen % 40)]   # (the image's last rows too: window 2)
                pl[row] = (True, b)
            q[row] = _near(rng, big[b])
        return q, pl

    def counts_lane(row):
        p0, p1 = UNITS[row // 128]
        return (row % 64) in (p1 if row % 128 >= 64 else p0)

    qi = len(imgs)
    q, pl = fill_big(128 * len(UNITS), counts_lane)
    imgs.append(q); pairs.append((BIG, qi)); plan[(BIG, qi)] = pl
    for name, n in SPLIT_ROWS.items():               # consecutive pairs of the same database image: their blocks share units
        qi = len(imgs)
        q, pl = fill_big(n, lambda row: row % 3 == 0 or row == n - 1)
        imgs.append(q); pairs.append((BIG, qi)); plan[(BIG, qi)] = pl

    # --- the small images: near-duplicates of their rows (the last one among them) between random rows
    for di, n in enumerate(DB_ROWS[:BIG]):
        qi = len(imgs)
        q = rng.integers(0, 256, (20, 128)).astype(np.uint8)
        pl = {}
        for row in range(0, 20, 2):
            b = (n - 1 - row // 2) % n
            q[row] = _near(rng, imgs[di][b])
            pl[row] = (n >= 2, b)                    # (an image of one row has no second neighbour: the reference reports nothing)
        imgs.append(q); pairs.append((di, qi)); plan[(di, qi)] = pl

    # --- CELL against SKEW. Even rows: rank = row; the cell of rank k holds the ranks of its window with (rank % 16) // 2 == (k % 16) // 2
    cell = [("near", 0, 1, 8, 2), ("accept", 3, 2, 9, 0), ("near2", 4, 20, 8, 2), ("acc2", 7, 22, 9, 0), ("tie", 10, 11, 0, 0), ("tie2", 8, 24, 0, 0)]
    qi = len(imgs)
    q = rng.integers(0, 256, (33, 128)).astype(np.uint8)
    pl = {}
    for k, (kind, b, u, n_two, n_one) in enumerate(cell):
        assert (b % 16) // 2 == (u % 16) // 2 and b < SKEW_EVEN and u < SKEW_EVEN
        row = 2 * k + 1
        qrow, used = _steps(rng, skew[b], D0 // 4)
        q[row] = qrow
        skew[u], _ = _steps(rng, skew[b], n_two, n_one, avoid=used)      # d(q, u) = D0 + 4 n_two + n_one
        pl[row] = (kind in ("accept", "acc2"), b)
    for k, b in enumerate(range(SKEW_EVEN, 40)):                         # winners in the odd half
        q[20 + 4 * k] = _near(rng, skew[b])
        pl[20 + 4 * k] = (True, b)
    assert np.array_equal(_odd(skew), np.arange(40) >= SKEW_EVEN)
    imgs.append(q); pairs.append((SKEW, qi)); plan[(SKEW, qi)] = pl

    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs), np.ascontiguousarray(np.array(pairs, np.uint32)), plan


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


def n_candidates():
    _, _, plan = images()
    return sum(len(pl) for (i, _), pl in plan.items() if len(images()[0][i]) >= 2)   # (no work against an image of one row)


def inputs_are_what_they_claim():
    """the inputs cannot drift away from the cases"""
    imgs, pairs, plan = images()
    ref = reference()
    # the reference accepts exactly the planted queries the plan calls accepted, with the planted row; no other query matches
    for (i, j) in map(tuple, pairs):
        m = ref.get((int(i), int(j)), np.zeros((0, 2), np.uint32))
        want = {row: b for row, (accept, b) in plan[(i, j)].items() if accept}
        assert {int(b): int(a) for a, b in m} == want, (i, j)
    # candidates per part of the units of COUNTS, and the lanes the cases name
    per_part = [(len(a), len(b)) for a, b in UNITS]
    assert per_part == [(0, 0), (1, 0), (4, 0), (5, 0), (7, 6), (64, 0), (0, 64), (64, 64), (60, 9), (0, 2)]
    assert set(UNITS[2][0]) == {0, 15, 16, 63}
    counts = plan[(BIG, SKEW + 1)]
    assert len(imgs[SKEW + 1]) == 128 * len(UNITS) and len(counts) == sum(a + b for a, b in per_part)
    assert sum(not a for a, _ in counts.values()) >= 60                     # rejected candidates between the accepted ones
    # the accepted winners of the 530-row image lie in both halves and in all three windows (the third one: 17 tiles, in the longer half)
    odd = _odd(imgs[BIG])
    rank = np.where(odd, np.cumsum(odd) - 1, np.cumsum(~odd) - 1)
    where = {(bool(odd[b]), int(rank[b]) // 128) for a, b in counts.values() if a}
    assert {h for h, _ in where} == {False, True} and {w for _, w in where} == {0, 1, 2}, where
    # units of two pairs: 3 blocks of HEAD + 5 of TAIL, its other 5 + 3 of MID, its other 2 + the 4 of LAST
    assert [-(-SPLIT_ROWS[k] // 16) for k in ("HEAD", "TAIL", "MID", "LAST")] == [3, 10, 5, 4]
    for k in range(2, 6):
        assert any(a for a, _ in plan[(BIG, SKEW + k)].values()) and tuple(pairs[k - 1]) == (BIG, SKEW + k)
    # the exact cases: distances as planned
    sk, q = imgs[SKEW].astype(np.int64), imgs[-1].astype(np.int64)
    d = ((q[:, None, :] - sk[None, :, :]) ** 2).sum(axis=2)
    two = np.sort(d, axis=1)[:, :2]
    assert [tuple(two[r]) for r in (1, 3, 5, 7, 9, 11)] == [(64, 98), (64, 100), (64, 98), (64, 100), (64, 64), (64, 64)]
    assert not np.float32(64) < R2 * np.float32(98) and np.float32(64) < R2 * np.float32(100) and not 64 < 0.64 * 100
    return ref


def lists_of(off, ij, pairs):
    return {k: v for k, v in _oracle.offsets_to_dict(pairs, off, ij).items() if len(v)}


def context(batch_pairs=None, profile=None):
    """the default kernel (variant 4, every stage, the 16x16x64 filter)"""
    imgs, _, _ = images()
    ctx = matching.MatchContext(0)
    ctx.set_option("variant", 4); ctx.set_option("stage", 3); ctx.set_option("filter_shape", 16)
    if batch_pairs:
        ctx.set_option("batch_pairs", batch_pairs)
    if profile:
        ctx.set_option("profile", profile)
    ctx.set_regions(list(imgs))
    return ctx


def _same(off, ij, pairs, what):
    got, want = lists_of(off, ij, pairs), {k: v for k, v in reference().items() if len(v)}
    assert got.keys() == want.keys(), what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


def check_lists_and_candidates():
    """one batch: the lists, and the candidates the filter handed over are exactly the planted queries ("profile" 2 counts them)"""
    _, pairs, _ = images()
    ctx = context(profile=2)
    try:
        st, off, ij = ctx.run(pairs, R2)          # (raises when the error flag is not zero)
    finally:
        ctx.close()
    _same(off, ij, pairs, "one batch")
    assert int(st.kernel_vgprs) == n_candidates()


def check_repeated_and_interleaved():
    """two batches per run on one context (both batch slots' best[] and cd[] hold what the run before left), the whole set twice, and a
    run of the 32x32x32 filter between them: that one is followed by l2_verify_kernel<false> and numbers best[] by parity slots"""
    _, pairs, _ = images()
    ctx = context(batch_pairs=-(-len(pairs) // 2))
    try:
        for shape in (16, 32, 16):
            ctx.set_option("filter_shape", shape)
            _, off, ij = ctx.run(pairs, R2)
            _same(off, ij, pairs, shape)
    finally:
        ctx.close()
