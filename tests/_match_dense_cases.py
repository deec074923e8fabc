"""Inputs and checks of the dense query layout of the default matching filter (l2_filter16_kernel reads its query fragments from a second
tile set that keeps an image's rows in their original order, ceil(n / 32) tiles per image; the database side keeps the tiles that are split
by norm parity, ceil(max(n_even, n_odd) / 16) per image). Shared by the GPU test and by the CPU test that runs the same
device source under the HIP emulation. The images are the smallest at which the two tile counts, the unit boundaries and the slot
numbering of best[] can go wrong; the reference lists are computed once per pair list and shared.

Lists are integers and are compared entry by entry: against the compiled reference (oracle/_ref) where it was built, else against its C
restatement. MatchContext.run raises when the verify stage's error flag is not zero (a slot of best[] read through the wrong layout holds
another query's code and trips it), so "run() returned" is "the flag is zero"."""
import functools

import numpy as np
import pytest

from openmvg_amd import _capi, matching, synth
from tests import _oracle
from tests._match_wave_cases import force_norm_parity

RATIO = 0.8
# index -> (rows, parity of the squared norms: None as they come, 0 / 1 all even / all odd, (p, k) all p except row k)
SPEC = [
    (1, None), (31, None), (32, None), (33, None), (127, None), (128, None), (129, None),   # tile and unit boundaries (a unit = 4 tiles = 128 rows)
    (0, None),              # an empty image: nJ = 0 as a query, nI < 2 as a database
    (128, 0),               # all even: 8 parity tiles (two units), 4 dense ones (one)
    (95, 1),                # all odd: 6 parity tiles, 3 dense ones (the last unit 3 tiles full)
    (64, (0, 40)),          # one odd row among even ones: 4 parity tiles, 2 dense ones
    (129, (1, 128)),        # one even row, the last, among odd ones: it alone occupies the fifth dense tile = the second unit
    (70, None),             # 3 dense tiles
]
BASE = 6                    # image 6 (129 rows): the others are noisy copies of its first rows, so that matches exist


def dense_tiles(n):
    return -(-n // 32)


def parity_tiles(d):
    odd = int((((d.astype(np.int64) - 128) ** 2).sum(axis=1) & 1).sum())
    return (max(odd, len(d) - odd) + 15) // 16


@functools.lru_cache(maxsize=None)
def images():
    sizes = [n for n, _ in SPEC]
    imgs = synth.random_descriptors(len(SPEC), sizes, seed=77)
    rng = np.random.default_rng(8)
    base = imgs[BASE].copy()
    for k, (n, par) in enumerate(SPEC):
        if k != BASE and n:
            m = min(n, len(base))
            shift = (3 * k) % max(1, len(base) - m + 1)      # not the identity map between query and database rows
            imgs[k][:m] = np.clip(base[shift:shift + m].astype(np.int16) + rng.integers(-9, 10, (m, 128)), 0, 255).astype(np.uint8)
        if par is None:
            continue
        p, lone = par if isinstance(par, tuple) else (par, None)
        imgs[k] = force_norm_parity(imgs[k], p)
        if lone is not None:
            imgs[k][lone, 0] ^= 1
    for d in imgs:
        d.setflags(write=False)
    return tuple(imgs)


def check_cases_are_what_they_claim():
    """the inputs cannot drift away from the cases they stand for"""
    imgs = images()
    pt = [parity_tiles(d) for d in imgs]
    dt = [dense_tiles(len(d)) for d in imgs]
    assert all(d <= p for d, p in zip(dt, pt))
    assert (pt[8], dt[8]) == (8, 4) and (pt[9], dt[9]) == (6, 3) and (pt[10], dt[10]) == (4, 2) and (pt[11], dt[11]) == (8, 5), (pt, dt)
    assert {t % 4 for t in dt if t} == {0, 1, 2, 3}, dt            # the last unit of an image 4, 1, 2 and 3 tiles full
    assert {len(d) % 32 for d in imgs} >= {0, 1, 31}                # a last tile full, one row and one row short
    odd = lambda d: (((d.astype(np.int64) - 128) ** 2).sum(axis=1) & 1)
    assert odd(imgs[8]).sum() == 0 and odd(imgs[9]).sum() == 95 and odd(imgs[10]).sum() == 1 and odd(imgs[11]).sum() == 128
    pairs = pair_list("both")
    n = np.array([len(d) for d in imgs])
    assert ((n[pairs[:, 1]] == 0).sum() > 0) and ((n[pairs[:, 0]] < 2).sum() > 0)      # skipped pairs inside the runs
    off, _ = reference("both")
    per = np.diff(off.astype(np.int64))
    assert not per[(n[pairs[:, 1]] == 0) | (n[pairs[:, 0]] < 2)].any()


def pair_list(kind):
    """sorted: the exhaustive list; both: it and its mirror, every image in both roles against every other"""
    p = matching.exhaustive_pairs_array(len(SPEC))
    if kind == "sorted":
        return p
    assert kind == "both"
    return np.ascontiguousarray(np.concatenate([p, p[:, ::-1]]))


@functools.lru_cache(maxsize=None)
def reference(kind):
    imgs, pairs = list(images()), pair_list(kind)
    off, ij = _oracle.port_matcher_regions_match(imgs, pairs, RATIO)
    if _oracle.have_ref_match():      # the compiled reference itself, brought into the same form
        per = _oracle.ref_matcher_regions_match(imgs, pairs, RATIO)
        lists = [per.get((int(i), int(j)), np.zeros((0, 2), np.uint32)) for i, j in pairs]
        off = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.uint64)
        ij = np.concatenate(lists).astype(np.uint32).reshape(-1, 2)
    assert int(off[-1]) > 1000          # equality with it is not vacuous
    off.setflags(write=False); ij.setflags(write=False)
    return off, ij


def context(filter_shape=16, batch_pairs=None):
    ctx = matching.MatchContext(0)
    ctx.set_option("variant", 4); ctx.set_option("stage", 3); ctx.set_option("filter_shape", filter_shape)
    if batch_pairs:
        ctx.set_option("batch_pairs", batch_pairs)
    ctx.set_regions(list(images()))
    return ctx


def _run(ctx, kind):
    _, off, ij = ctx.run(pair_list(kind), np.float32(RATIO) * np.float32(RATIO))
    return off, ij


def check_default_equals_reference(kind):
    want_off, want_ij = reference(kind)
    ctx = context()
    try:
        off, ij = _run(ctx, kind)
    finally:
        ctx.close()
    assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), kind


def check_batch_seams(batch_pairs, kind="both"):
    """batches so small that both batch slots are reused many times within a run, and a second run of the same context: every best[] slot
    the verify stage and the compaction read was written by this batch's filter launch, in the dense numbering"""
    want_off, want_ij = reference(kind)
    ctx = context(batch_pairs=batch_pairs)
    try:
        for run in (0, 1):
            off, ij = _run(ctx, kind)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), (batch_pairs, run)
    finally:
        ctx.close()


def check_cross_check_shapes(kind="both"):
    """the kernels that keep the parity-split query slots (filter_shape 32 and 17) give the same lists on the same inputs, and one context
    that alternates between the layouts - best[] then holds the other numbering's words from the run before - does too"""
    want_off, want_ij = reference(kind)
    ctx = context(batch_pairs=7)
    try:
        for shape in (32, 16, 17, 16):
            ctx.set_option("filter_shape", shape)
            off, ij = _run(ctx, kind)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), shape
    finally:
        ctx.close()


# (variant, filter_shape, stage, debug_filter). The matcher resolves the four options into one kernel form per run (the table above
# resolve_form in openmvg_amd/csrc/mvgx_match.hip, include/mvgx.h): every combination the filter accepts, and the exact kernel with the
# filter's options set, which it must ignore ...
FORMS_ALL = [(4, shape, stage, dbg) for shape in (16, 17, 32) for stage in (1, 2, 3) for dbg in (0, 8, 16)] + [(1, 17, 3, 16)]
# ... and, for the slow emulation, the rows of that table that no other test reaches: a 16x16x64 shape with register or builtin staging
# (the 32x32x32 filter runs), an earlier epilogue with shape 17 (the shape is ignored) and with stage 1 (the epilogue is)
FORMS_UNREACHED = [(4, 17, 1, 0), (4, 16, 2, 0), (4, 17, 3, 8), (4, 16, 1, 16), (1, 17, 3, 16)]


def check_form_resolution(forms, kind="sorted"):
    """every combination of the options reaches a kernel form whose lists equal the reference's, on one context: best[] holds the words of
    the run before, often in the other slot numbering, and each form reads only what its own filter launch wrote"""
    want_off, want_ij = reference(kind)
    ctx = context(batch_pairs=7)
    try:
        for variant, shape, stage, dbg in forms:
            for key, value in (("variant", variant), ("filter_shape", shape), ("stage", stage), ("debug_filter", dbg)):
                ctx.set_option(key, value)
            off, ij = _run(ctx, kind)
            assert np.array_equal(off, want_off) and np.array_equal(ij, want_ij), (variant, shape, stage, dbg)
    finally:
        ctx.close()


def check_debug_filter_values():
    """the option takes the three epilogue forms the library has and refuses everything else, the removed timing forms 1..7 included"""
    ctx = matching.MatchContext(0)
    try:
        for value in (0, 8, 16):
            ctx.set_option("debug_filter", value)
        for value in (1, 2, 3, 4, 5, 6, 7, 9, 17):
            with pytest.raises(_capi.MvgxError) as e:
                ctx.set_option("debug_filter", value)
            assert e.value.code == _capi.MVGX_ERR_ARG, value
    finally:
        ctx.close()


def check_env_filter_ignored(kind="sorted"):
    """call with MVGX_MATCH_FILTER=3 in the environment: the context is created all the same and runs the default form"""
    check_default_equals_reference(kind)
