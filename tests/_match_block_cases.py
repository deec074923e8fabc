"""Inputs and checks of the block-granular work list of the default matching filter (l2_filter16_kernel: a wave's unit is 8 consecutive
blocks of 16 query rows of the pairs that share the database image, up to two segments - the tail of one pair, the head of the next;
DESIGN.md 3.2). Shared by the GPU test and by the CPU test that runs the same device source under the HIP emulation. The images are the
smallest at which the packing can go wrong; the reference lists of a pair list are computed once and shared.

Results are integers and are compared for equality with _oracle.port_matcher_regions_match. Every run relies on the context's error flag
as tests/_match_wave_cases.py explains: a slot of best[] that this batch's filter did not write, or wrote for the wrong pair, trips it."""
import functools

import numpy as np

from openmvg_amd import matching, synth
from tests import _oracle

RATIO = 0.8
# index -> rows. The large images have 9 .. 16 blocks of 16 rows (every remainder mod 8), their last blocks hold 1, 8, 15, 16, 8, 16, 15
# and 1 rows, and 129, 175, 200 and 239 end in a dense tile without a second block (n mod 32 in 1..16). Images of 1, 0, 2, 15, 16 and 17
# rows sit between them: pairs without work (nI < 2, nJ = 0) inside a run of one database image, and images of one or two blocks that
# make a unit meet a third image.
SIZES = [129, 1, 152, 0, 175, 2, 192, 15, 200, 16, 224, 17, 239, 241]
LARGE = [0, 2, 4, 6, 8, 10, 12, 13]
TINY = [1, 3, 5, 7, 9, 11]


def blocks(n):
    return -(-n // 16)


@functools.lru_cache(maxsize=None)
def images():
    imgs = synth.random_descriptors(len(SIZES), SIZES, seed=43)
    rng = np.random.default_rng(8)
    for a, b in zip(LARGE[:-1], LARGE[1:]):   # near-duplicates between consecutive large images: matches exist
        m = min(SIZES[a], SIZES[b])
        imgs[b][:m] = np.clip(imgs[a][:m].astype(np.int16) + rng.integers(-9, 10, (m, 128)), 0, 255).astype(np.uint8)
    for t in TINY:                            # ... and between the tiny images and the tail of the first one
        m = SIZES[t]
        imgs[t][:m] = np.clip(imgs[0][-m or len(imgs[0]):].astype(np.int16) + rng.integers(-9, 10, (m, 128)), 0, 255).astype(np.uint8)
    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs)


def pair_list(kind):
    """sorted: the exhaustive list (runs of one database image, 91 pairs); both: it and its mirror; shuffled: those 182 pairs in a fixed
    random order, where almost every pair changes the database image - a workgroup must never mix two of them"""
    p = matching.exhaustive_pairs_array(len(SIZES))
    if kind == "sorted":
        return p
    both = np.ascontiguousarray(np.concatenate([p, p[:, ::-1]]))
    if kind == "both":
        return both
    assert kind == "shuffled"
    out = np.ascontiguousarray(both[np.random.default_rng(19).permutation(len(both))])
    assert int((out[1:, 0] != out[:-1, 0]).sum()) > 0.8 * len(out)
    return out


def units_of(pairs, batch_pairs=None):
    """the partition DESIGN.md 3.2 describes, restated for the assertions on the inputs: a list of units, each a list of segments
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


def inputs_cover_the_packing_cases():
    """the inputs cannot drift away from the cases"""
    assert {blocks(SIZES[k]) % 8 for k in LARGE} == set(range(8))
    assert {(SIZES[k] - 1) % 16 + 1 for k in LARGE} == {1, 8, 15, 16}                 # valid rows of the last block
    assert sorted(SIZES[k] for k in TINY) == [0, 1, 2, 15, 16, 17]
    units = units_of(pair_list("sorted"))
    two = [u for u in units if len(u) == 2]
    assert {u[0][3] for u in two} == set(range(1, 8))                                 # every split point
    assert all(u[1][2] == 0 for u in two)                                             # the second segment starts at block 0
    ends = lambda s: s[2] + s[3] == blocks(SIZES[s[1]])
    assert any(len(u) == 1 and u[0][3] == 8 and ends(u[0]) and u[0][2] > 0 for u in units)   # a pair's blocks end a unit exactly
    # the last dense tile of JA has no second block, and the next image's block 0 follows in the same unit
    assert any(0 < SIZES[u[0][1]] % 32 <= 16 and ends(u[0]) for u in two)
    # closed early because a third image would enter: two segments, fewer than 8 blocks, and the next unit goes on with the same I
    pairs = pair_list("sorted")
    early = [i for i, u in enumerate(units[:-1]) if len(u) == 2 and u[0][3] + u[1][3] < 8 and pairs[units[i + 1][0][0]][0] == pairs[u[0][0]][0]]
    assert early
    # a pair without work between the two segments of one unit
    assert any(u[1][0] - u[0][0] > 1 for u in two)
    # database images of 0 and 1 rows head runs without work; one of 2 rows heads a run with work
    assert any(SIZES[i] == 2 and SIZES[j] > 0 for i, j in pairs) and any(SIZES[i] < 2 for i, j in pairs)
    # batches of 3 and 8 pairs close units in the middle of a run
    for bp in (3, 8):
        cut = units_of(pairs, bp)
        assert len(cut) > len(units) and any(sum(s[3] for s in u) < 8 and len(u) == 1 for u in cut)
    return units


@functools.lru_cache(maxsize=None)
def reference(kind):
    off, ij = _oracle.port_matcher_regions_match(list(images()), pair_list(kind), RATIO)
    assert int(off[-1]) > 500          # equality with it is not vacuous
    tiny_j = [k for k, (i, j) in enumerate(pair_list(kind)) if j in TINY]
    assert sum(int(off[k + 1] - off[k]) for k in tiny_j) > 10   # ... also in the tiny images
    off.setflags(write=False); ij.setflags(write=False)
    return off, ij


R2 = np.float32(RATIO) * np.float32(RATIO)


def context(batch_pairs=None, profile=None):
    """the default kernel (variant 4, every stage, the 16x16x64 filter)"""
    ctx = matching.MatchContext(0)
    ctx.set_option("variant", 4); ctx.set_option("stage", 3); ctx.set_option("filter_shape", 16)
    if batch_pairs:
        ctx.set_option("batch_pairs", batch_pairs)
    if profile:
        ctx.set_option("profile", profile)
    ctx.set_regions(list(images()))
    return ctx


def check_pair_order(kind):
    want_off, want_ij = reference(kind)
    ctx = context()
    try:
        _, off, ij = ctx.run(pair_list(kind), R2)     # (raises when the error flag is not zero)
    finally:
        ctx.close()
    assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), kind


def check_batch_boundaries(batch_pairs):
    """units are closed in the middle of a run of one database image, and the two batch slots' best[] buffers are reused while they hold
    other pairs' codes: the second run of the same context meets what the first one left in both"""
    want_off, want_ij = reference("sorted")
    ctx = context(batch_pairs)
    try:
        for run in (0, 1):
            _, off, ij = ctx.run(pair_list("sorted"), R2)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), (batch_pairs, run)
    finally:
        ctx.close()


def check_mixed_filters():
    """the parity-slot filters (the 32x32x32 kernel, the half-window 16x16x64 kernel) run on the same context between runs of the default
    one: they number best[] differently and leave their own codes in it"""
    want_off, want_ij = reference("sorted")
    ctx = context(8)
    try:
        for shape in (16, 32, 16, 17, 16):
            ctx.set_option("filter_shape", shape)
            _, off, ij = ctx.run(pair_list("sorted"), R2)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), shape
    finally:
        ctx.close()


def check_candidate_count():
    """ "profile" 2 counts the candidates over the blocks of the units: the count does not depend on where the batches end nor on what
    earlier batches left in best[], and lies between the matches and the queries with work"""
    pairs = pair_list("sorted")
    want_off, want_ij = reference("sorted")
    counts = []
    for batch_pairs, runs in ((5, 2), (None, 1)):
        ctx = context(batch_pairs, profile=2)
        try:
            for _ in range(runs):
                st, off, ij = ctx.run(pairs, R2)
                assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij)
                counts.append(int(st.kernel_vgprs))
        finally:
            ctx.close()
    assert len(set(counts)) == 1 and len(want_ij) <= counts[0] <= sum(SIZES[j] for i, j in pairs if SIZES[i] >= 2), counts


def records_cases_text():
    """the image sizes and pair lists of this module for tests/native/match_records_main.cpp"""
    lines = [str(len(SIZES)), " ".join(map(str, SIZES))]
    for kind in ("sorted", "both", "shuffled"):
        p = pair_list(kind)
        for bp in (len(p), 3, 8):
            lines.append(f"{bp} {len(p)} " + " ".join(map(str, p.reshape(-1))))
    return "\n".join(lines) + "\n"
