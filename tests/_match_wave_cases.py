"""Inputs and checks of the wave-packed work list of the default matching filter (l2_filter16_kernel: units of four query tiles, one per
wave, four to a workgroup across the pairs that share the database image). Shared by the GPU test and by the CPU test that
runs the same device source under the HIP emulation. The images are the smallest at which the partition can go wrong; the reference
lists of a pair list are computed once and shared.

The context's error flag: l2_verify_kernel recomputes every candidate's best distance and counts a disagreement with the filter's d0;
mvgx_match_run returns MVGX_ERR_NUMERIC (MatchContext.run raises) when that count is not zero. A slot of best[] that the filter launch
of this batch did not write holds the code of another pair's candidate and trips it, so "run() returned" is "the flag is zero"."""
import functools

import numpy as np

from openmvg_amd import matching, synth
from tests import _oracle

RATIO = 0.8
# index -> rows. The large images give 5 to 17 query tiles: 2 to 5 wave units, the last one 1 to 4 tiles full (checked by
# unit_counts_cover_every_remainder). Images of 0, 1 and 2 rows sit between them, so that pairs without work (nI < 2 or nJ = 0) and
# pairs of one tile fall inside a run of pairs with the same database image. The last image has rows of even squared norm only.
SIZES = [130, 0, 150, 1, 260, 2, 400, 530, 170, 210, 192]
LARGE = [0, 2, 4, 6, 7, 8, 9, 10]
EVEN = 10


def force_norm_parity(d, parity):
    """flips the LSB of byte 0 where needed, so that every row's sum (a - 128)^2 has the given parity"""
    d = d.copy()
    odd = (((d.astype(np.int64) - 128) ** 2).sum(axis=1) & 1).astype(bool)
    d[odd != bool(parity), 0] ^= 1
    return d


def tiles(d):
    """tiles of an image in the device layout: 16 even-norm and 16 odd-norm slots per tile"""
    odd = int((((d.astype(np.int64) - 128) ** 2).sum(axis=1) & 1).sum())
    return (max(odd, len(d) - odd) + 15) // 16


@functools.lru_cache(maxsize=None)
def images():
    imgs = synth.random_descriptors(len(SIZES), SIZES, seed=41)
    rng = np.random.default_rng(6)
    for a, b in zip(LARGE[:-1], LARGE[1:]):   # near-duplicates between consecutive large images: matches exist
        m = min(SIZES[a], SIZES[b])
        imgs[b][:m] = np.clip(imgs[a][:m].astype(np.int16) + rng.integers(-9, 10, (m, 128)), 0, 255).astype(np.uint8)
    imgs[EVEN] = force_norm_parity(imgs[EVEN], 0)
    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs)


def unit_counts_cover_every_remainder():
    """the inputs cannot drift away from the cases: ceil(nt / 4) mod 4 takes all four values (a pair's units end a record exactly, or
    leave 1, 2, 3 waves to the next pair), and the all-even image has nt = n / 16 (half of every tile is padding)"""
    imgs = images()
    nt = {k: tiles(imgs[k]) for k in LARGE}
    assert {-(-t // 4) % 4 for t in nt.values()} == {0, 1, 2, 3}, nt
    assert {t % 4 for t in nt.values()} == {0, 1, 2, 3}, nt          # the last unit 4, 1, 2 and 3 tiles full
    assert nt[EVEN] == -(-SIZES[EVEN] // 16) and tiles(imgs[5]) == 1 and tiles(imgs[1]) == 0, nt
    return nt


def pair_list(kind):
    """sorted: the exhaustive list (runs of one database image, 55 pairs); both: it and its mirror; shuffled: those 110 pairs in a fixed random
    order, where almost every pair changes the database image - a workgroup must never mix two of them"""
    p = matching.exhaustive_pairs_array(len(SIZES))
    if kind == "sorted":
        return p
    both = np.ascontiguousarray(np.concatenate([p, p[:, ::-1]]))
    if kind == "both":
        return both
    assert kind == "shuffled"
    out = np.ascontiguousarray(both[np.random.default_rng(17).permutation(len(both))])
    assert int((out[1:, 0] != out[:-1, 0]).sum()) > 0.8 * len(out)
    return out


@functools.lru_cache(maxsize=None)
def reference(kind):
    off, ij = _oracle.port_matcher_regions_match(list(images()), pair_list(kind), RATIO)
    assert int(off[-1]) > 1000          # equality with it is not vacuous
    off.setflags(write=False); ij.setflags(write=False)
    return off, ij


def context(batch_pairs=None, profile=None):
    """the default kernel (variant 4, every stage, the 16x16x64 filter), as tests.test_matching_gpu.run_hip selects it for 43"""
    ctx = matching.MatchContext(0)
    ctx.set_option("variant", 4); ctx.set_option("stage", 3); ctx.set_option("filter_shape", 16)
    if batch_pairs:
        ctx.set_option("batch_pairs", batch_pairs)
    if profile:
        ctx.set_option("profile", profile)
    ctx.set_regions(list(images()))
    return ctx


def check_pair_order(kind, run_hip):
    want_off, want_ij = reference(kind)
    _, off, ij = run_hip(list(images()), pair_list(kind), RATIO, 43)     # (raises when the error flag is not zero)
    assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), kind


def check_batch_boundaries(batch_pairs):
    """records are closed in the middle of a run of one database image, and the two batch slots' best[] buffers are reused while they hold
    other pairs' codes: the second run of the same context meets what the first one left in both"""
    want_off, want_ij = reference("sorted")
    ctx = context(batch_pairs)
    try:
        for run in (0, 1):
            _, off, ij = ctx.run(pair_list("sorted"), np.float32(RATIO) * np.float32(RATIO))
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), (batch_pairs, run)
    finally:
        ctx.close()


def check_candidate_count():
    """ "profile" 2 counts the candidates over the units of the records: the count does not depend on where the batches end nor on what
    earlier batches left in best[] (a sweep over all of best[] would), and lies between the matches and the queries"""
    pairs = pair_list("sorted")
    want_off, want_ij = reference("sorted")
    r2 = np.float32(RATIO) * np.float32(RATIO)
    counts = []
    for batch_pairs, runs in ((5, 2), (None, 1)):
        ctx = context(batch_pairs, profile=2)
        try:
            for _ in range(runs):
                st, off, ij = ctx.run(pairs, r2)
                assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij)
                counts.append(int(st.kernel_vgprs))
        finally:
            ctx.close()
    assert len(set(counts)) == 1 and len(want_ij) <= counts[0] <= sum(SIZES[j] for i, j in pairs if SIZES[i] >= 2), counts
