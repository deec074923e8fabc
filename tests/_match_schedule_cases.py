"""Inputs and checks of the two host decisions around the matching filter's launches: the batches of a run with ramps at its two ends
(option "batch_ramp", mvgx_records::batch_schedule) and the order of the records inside an XCD's slice (option "record_order",
mvgx_records::order_records). Shared by the GPU test and by the CPU test that runs the same source under the HIP
emulation. Neither decision may change a list: results are integers and are compared for equality with
_oracle.port_matcher_regions_match, computed once. MatchContext.run raises when the context's error flag is not zero.

40 images of 0 .. 130 descriptors. The ramped runs take the 315 pairs of every image with its next nine (the emulated device is slow;
a ramp needs 256 pairs, four batches' worth, and 288 for both devices of a pair to get one): with "batch_pairs" 64 and "batch_ramp" 8 the run starts on batches of 8, 16 and 32 pairs
and ends on 32, 16 and 8 (each twice on two devices), and a batch holds up to eight database images. The one-batch case takes all 780
sorted pairs. The images hold 83 dense query tiles, less than one chunk of the record order, so the tests set "record_chunk_tiles" 4:
the order then has some 20 keys and moves records wherever a slice holds two database images."""
import functools

import numpy as np

from openmvg_amd import matching, synth
from tests import _oracle

RATIO = 0.8
R2 = np.float32(RATIO) * np.float32(RATIO)
B, FLOOR = 64, 8
# ragged: no row, one row (no database image), two rows (the smallest database image), 17 rows (a second block of one row); the rest 20 .. 130
SIZES = [97, 0, 130, 1, 64, 2, 113, 17, 20, 128] + [20 + (37 * k) % 111 for k in range(30)]
assert len(SIZES) == 40 and min(SIZES[10:]) >= 20 and max(SIZES) == 130


@functools.lru_cache(maxsize=None)
def images():
    imgs = synth.image_descriptors(len(SIZES), n_desc=max(SIZES), seed=61)
    imgs = [np.ascontiguousarray(d[:s]) for d, s in zip(imgs, SIZES)]
    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs)


@functools.lru_cache(maxsize=None)
def pairs(kind="near"):
    p = matching.exhaustive_pairs_array(len(SIZES))
    if kind == "near":
        p = np.ascontiguousarray(p[p[:, 1] - p[:, 0] <= 9])
        assert B + 2 * 2 * (8 + 16 + 32) <= len(p) == 315
    else:
        assert kind == "all"
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(kind="near"):
    off, ij = _oracle.port_matcher_regions_match(list(images()), pairs(kind), RATIO)
    assert int(off[-1]) > 1000          # equality with it is not vacuous
    off.setflags(write=False); ij.setflags(write=False)
    return off, ij


def context(devices=None, record_order=1, batch_pairs=B):
    ctx = matching.MatchContext(0) if devices is None else matching.MatchContext(devices=devices)
    if batch_pairs:
        ctx.set_option("batch_pairs", batch_pairs)
    ctx.set_option("batch_ramp", FLOOR)
    ctx.set_option("record_order", record_order)
    ctx.set_option("record_chunk_tiles", 4)
    ctx.set_regions(list(images()))
    return ctx


def expected_sizes(nd):
    """the schedule of the 315 pairs at B = 64, restated: the ramps, and what is left in equal batches of at most B"""
    ramp = [8] * nd + [16] * nd + [32] * nd
    mid = len(pairs()) - 2 * sum(ramp)
    n_mid = -(-mid // B)
    return ramp + [mid // n_mid + (k < mid % n_mid) for k in range(n_mid)] + ramp[::-1]


def check_ramped_run(devices, record_order):
    """the collecting run twice on one context, first with the other record order (both slots' buffers reused: they were sized on the
    small first batches), the streamed run against the schedule, and a sink that stops"""
    want_off, want_ij = reference()
    nd = len(devices) if devices else 1
    ctx = context(devices, 1 - record_order)
    try:
        sched = ctx.batch_schedule(len(pairs()))
        assert [nb for _, nb in sched] == expected_sizes(nd) and sched[0][1] == FLOOR, sched
        assert [p0 for p0, _ in sched] == [int(x) for x in np.cumsum([0] + [nb for _, nb in sched[:-1]])]
        for run in (0, 1):
            _, off, ij = ctx.run(pairs(), R2)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), (devices, record_order, run)
            ctx.set_option("record_order", record_order)
        seen = []
        counts = np.zeros(len(pairs()) + 1, np.uint64)
        pieces = {}

        def on_batch(p0, off, lists):
            seen.append((p0, len(off) - 1))
            counts[p0 + 1:p0 + len(off)] = np.diff(off.astype(np.int64)).astype(np.uint64)
            pieces[p0] = lists.copy()

        st = ctx.run_stream(pairs(), R2, on_batch)
        assert sorted(seen) == sched and len(seen) == len(sched), (seen, sched)     # every batch of the schedule exactly once ...
        if nd == 1:
            assert seen == sched                                                   # ... and in order on one device
        assert np.array_equal(np.cumsum(counts, dtype=np.uint64), want_off)
        assert np.array_equal(np.concatenate([pieces[k] for k in sorted(pieces)]), want_ij)
        assert st.n_matches == len(want_ij)
        # a sink that asks to stop is not entered again
        stopped = []
        ctx.run_stream(pairs(), R2, lambda p0, off_, ij_: stopped.append(p0) or True)
        assert len(stopped) == 1
        # without the ramp the same context cuts steps of exactly B again
        ctx.set_option("batch_ramp", 0)
        assert ctx.batch_schedule(len(pairs())) == [(p0, min(B, len(pairs()) - p0)) for p0 in range(0, len(pairs()), B)]
    finally:
        ctx.close()


def check_one_batch_slices_of_several_database_images(record_order):
    """the whole sorted list in one batch: 39 runs of one database image over 8 slices, so every slice holds several and the order moves
    records in all of them; "profile" 2 walks the same list for the candidate count, which may not depend on the order"""
    want_off, want_ij = reference("all")
    ctx = context(None, record_order, batch_pairs=None)
    ctx.set_option("profile", 2)
    try:
        assert ctx.batch_schedule(len(pairs("all"))) == [(0, len(pairs("all")))]
        st, off, ij = ctx.run(pairs("all"), R2)
        assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), record_order
        return int(st.kernel_vgprs)
    finally:
        ctx.close()
