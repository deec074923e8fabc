"""State kept between calls, emulated (the GPU twin is tests/test_adapter_kept_context_gpu.py).

Matcher_Regions::Match keeps its SIFT match context - device scratch, page-locked result buffers, held stream batches - from one
call to the next (openmvg_amd/adapter/mvgx_matcher_regions.cpp, KeptMatchContext); the next call uploads its own regions into it
through mvgx_match_set_regions, which reuses whatever fits. One call sequence through the SIFT route grows, shrinks and reorders
the image set on that kept context, changes the batch size, interleaves the other routes, releases the context and (here) injects
a failure; every step's container must equal the restatement, the reference TU where oracle/_ref exists, and the same call with
MVGX_ADAPTER_KEEP_CONTEXT=0 (a context per call), and every step runs under the route check of tests/_adapter_route.py.

The library-level twin re-uses ONE MatchContext / HammingContext / L2fContext / L2u8Context / CascadeContext across image sets and
compares every run with a fresh context and the restatement."""
import threading

import numpy as np
import pytest

from openmvg_amd import matching, synth
from tests import _emu, _oracle
from tests._adapter_route import counters, device_route
from tests.test_l2u8_cpu import liop_like

# mvgx_match_run's scratch cap (mvgx_match.hip, batch_size): a batch holds at most max(16, 2^29 / qstride) pairs, qstride = 32 rows per
# padded tile of the largest image's larger norm-parity class (16 rows per tile). Against the adapter's default of 16 384 pairs the
# cap binds once qstride > 2^15, i.e. once one parity class of one image has more than 16 384 rows: an image of 32 769 rows has one
# for certain, whatever the split of its rows.
CAP_ROWS = 32769


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _truncate(full, counts):
    return [full[k][:int(n)] for k, n in enumerate(counts)]


def image_sets(big):
    """the SIFT sets of the sequence; `big`: (images, rows) of B and the row counts of C"""
    a_full = synth.image_descriptors(7, n_desc=450, seed=11)
    A = _truncate(a_full, [450, 450, 450, 0, 450, 1, 450])     # the set of test_matcher_regions_replacement_equals_reference
    nb, rows_b, rows_c = big
    B = synth.image_descriptors(nb, n_desc=rows_b, seed=13)
    c_full = synth.image_descriptors(len(rows_c), n_desc=max(rows_c), seed=17)
    C = _truncate(c_full, rows_c)
    # A's images with the row counts permuted: image 0 (450 rows) becomes one row, image 2 empty, the empty image 3 and the one-row
    # image 5 full - rows, tiles or parity classes left over from an earlier upload would produce matches
    D = _truncate(a_full, [1, 450, 0, 450, 450, 450, 450])
    return A, B, C, D


def sift_step(lib, descs, monkeypatch, reference=True):
    """one SIFT call on the kept context: container == restatement == reference TU == the same call without the kept context"""
    pairs = matching.exhaustive_pairs_array(len(descs))
    with device_route(lib, len(pairs), monkeypatch):   # every view is SIFT_Regions (empty ones included): every pair on the device
        got = _oracle.ref_matcher_regions_match(descs, pairs, 0.8, lib=lib)
    off, ij = _oracle.port_matcher_regions_match(descs, pairs, 0.8)
    _same(got, _oracle.offsets_to_dict(pairs, off, ij))
    if reference and _oracle.have_ref_match():
        _same(got, _oracle.ref_matcher_regions_match(descs, pairs, 0.8))
    with monkeypatch.context() as m:
        m.setenv("MVGX_ADAPTER_KEEP_CONTEXT", "0")
        with device_route(lib, len(pairs), monkeypatch):
            fresh = _oracle.ref_matcher_regions_match(descs, pairs, 0.8, lib=lib)
    _same(got, fresh)
    return got


def other_routes(lib, monkeypatch):
    """a Hamming, a float and a LIOP call between two SIFT steps (own contexts, created and destroyed per call)"""
    sizes = [100, 0, 90, 1, 2]
    pairs = matching.exhaustive_pairs_array(len(sizes))
    b = synth.binary_descriptors(len(sizes), sizes, seed=9)
    with device_route(lib, len(pairs), monkeypatch):
        got = _oracle.ref_matcher_regions_match_binary64(b, pairs, 0.8, lib=lib)
    _same(got, _oracle.offsets_to_dict(pairs, *_oracle.port_matcher_regions_match_hamming(b, pairs, 0.8)))
    f = synth.float_descriptors(len(sizes), sizes, seed=9)
    with device_route(lib, len(pairs), monkeypatch):
        got = _oracle.ref_matcher_regions_match_float64(f, pairs, 0.8, lib=lib)
    _same(got, _oracle.offsets_to_dict(pairs, *_oracle.port_matcher_regions_match_f32(f, pairs, 0.8)))
    lp = liop_like(sizes, 144, seed=21)
    with device_route(lib, len(pairs), monkeypatch):
        got = _oracle.ref_matcher_regions_match_liop144(lp, pairs, 0.8, lib=lib)
    _same(got, _oracle.offsets_to_dict(pairs, *_oracle.port_matcher_regions_match(lp, pairs, 0.8, dim=144)))


def concurrent_calls(lib, sets):
    """two Python threads in Match() (ctypes releases the GIL), started together: when the calls overlap, one holds the kept context
    and the other makes its own; nothing here proves that they did overlap - either way both containers and the counters must be right"""
    results, errors = [None, None], []

    def call(k):
        try:
            results[k] = _oracle.ref_matcher_regions_match(sets[k], matching.exhaustive_pairs_array(len(sets[k])), 0.8, lib=lib)
        except BaseException as e:   # (re-raised on the test's thread)
            errors.append(e)

    counters(lib, reset=True)
    start = threading.Barrier(2)

    def call_together(k):
        start.wait()
        call(k)

    threads = [threading.Thread(target=call_together, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    n = [len(matching.exhaustive_pairs_array(len(s))) for s in sets]
    assert counters(lib, reset=True) == (n[0] + n[1], 0, 0)
    for k in range(2):
        pairs = matching.exhaustive_pairs_array(len(sets[k]))
        _same(results[k], _oracle.offsets_to_dict(pairs, *_oracle.port_matcher_regions_match(sets[k], pairs, 0.8)))


def kept_context_sequence(lib, monkeypatch, big, inject=False):
    """A -> other routes -> B -> C -> D -> E -> F -> release -> (injected failure) -> two threads, all on the process's kept context"""
    A, B, C, D = image_sets(big)
    monkeypatch.delenv("MVGX_ADAPTER_KEEP_CONTEXT", raising=False)
    monkeypatch.delenv("MVGX_ADAPTER_BATCH_PAIRS", raising=False)
    sift_step(lib, A, monkeypatch)
    other_routes(lib, monkeypatch)
    sift_step(lib, B, monkeypatch)                                 # grow: more images, more rows
    # query stride beyond one batch slot's default scratch; the reference TU is left out here only for its CPU time (brute force over
    # 34 000 x 9 000 rows on the host) - the restatement and the per-call context still check every list
    sift_step(lib, C, monkeypatch, reference=False)
    sift_step(lib, D, monkeypatch)                                 # back to A's images, row counts permuted
    other_routes(lib, monkeypatch)
    sift_step(lib, [d[:0] for d in A], monkeypatch)                # every image empty
    sift_step(lib, A[:1], monkeypatch)                             # one image: no pair, no device call
    sift_step(lib, A, monkeypatch)
    for batch in ("5", None, str(2 ** 20 + 1), "3"):               # batch sizes on the kept context (2^20 + 1: clamped to the library's 2^20)
        if batch is None:
            monkeypatch.delenv("MVGX_ADAPTER_BATCH_PAIRS")
        else:
            monkeypatch.setenv("MVGX_ADAPTER_BATCH_PAIRS", batch)
        sift_step(lib, B if batch == "3" else A, monkeypatch)
    monkeypatch.delenv("MVGX_ADAPTER_BATCH_PAIRS")
    assert lib.mvgx_adapter_match_release_context() == 1
    sift_step(lib, D, monkeypatch)                                 # a new kept context after the release
    if inject:
        # a failing run destroys the kept context: that call finishes on the reference route, the next one makes a new context
        pairs = matching.exhaustive_pairs_array(len(A))
        want = _oracle.offsets_to_dict(pairs, *_oracle.port_matcher_regions_match(A, pairs, 0.8))
        counters(lib, reset=True)
        with monkeypatch.context() as m:
            m.setenv("MVGX_ADAPTER_INJECT_FAILURE", "match:run")
            _same(_oracle.ref_matcher_regions_match(A, pairs, 0.8, lib=lib), want)
        assert counters(lib, reset=True) == (0, len(pairs), 1)
        sift_step(lib, B, monkeypatch)
    concurrent_calls(lib, (A, D))
    sift_step(lib, A, monkeypatch)


def _lib():
    lib = _oracle.adapter_emu()
    if lib is None:
        pytest.skip("openMVG tree / adapter objects not present")
    return lib


def test_kept_context_sequence_emulated(monkeypatch):
    """the sequence on the emulated adapter. Sizes: B is 10 images x 600 rows (the GPU twin's 30 x 700 is minutes under emulation);
    C is one image of CAP_ROWS = 32 769 rows, one of a single row and one of 60 rows - the smallest image that crosses the scratch cap
    of mvgx_match_run at the adapter's default batch size, with a neighbour too small to make the pair count matter"""
    kept_context_sequence(_lib(), monkeypatch, (10, 600, [CAP_ROWS, 1, 60]), inject=True)


# ---- the library-level twin: one context, several image sets ----
def _sift_sets():
    A, B, _, D = image_sets((10, 600, [1]))
    return [A, B, D, A]


def match_context_reuse():
    ctx = matching.MatchContext(0)
    try:
        for descs in _sift_sets():
            pairs = matching.exhaustive_pairs_array(len(descs))
            ctx.set_regions(descs)
            _, off, ij = ctx.run(pairs, np.float32(0.8) * np.float32(0.8))
            fresh = matching.MatchContext(0)
            try:
                fresh.set_regions(descs)
                _, f_off, f_ij = fresh.run(pairs, np.float32(0.8) * np.float32(0.8))
            finally:
                fresh.close()
            o_off, o_ij = _oracle.port_matcher_regions_match(descs, pairs, 0.8)
            assert np.array_equal(off, f_off) and np.array_equal(ij, f_ij)
            assert np.array_equal(off, o_off) and np.array_equal(ij, o_ij)
    finally:
        ctx.close()


def _other_sets(kind):
    """(context class, image sets A -> B -> D -> A, restatement, ratio argument) of the Hamming / float / uint8-144 routes"""
    def grow_shrink(make):
        a_full = make([120, 120, 120, 120, 120])
        a = _truncate(a_full, [120, 0, 90, 1, 2])
        b = make([150] * 8)
        d = _truncate(a_full, [1, 120, 2, 90, 0])
        return [a, b, d, a]
    if kind == "hamming":
        return (matching.HammingContext, grow_shrink(lambda s: synth.binary_descriptors(len(s), s, seed=9)),
                lambda d, p: _oracle.port_matcher_regions_match_hamming(d, p, 0.8), np.float32(0.8))
    if kind == "l2f":
        return (matching.L2fContext, grow_shrink(lambda s: synth.float_descriptors(len(s), s, seed=9)),
                lambda d, p: _oracle.port_matcher_regions_match_f32(d, p, 0.8), np.float32(0.8) * np.float32(0.8))
    return (matching.L2u8Context, grow_shrink(lambda s: liop_like(s, 144, seed=21)),
            lambda d, p: _oracle.port_matcher_regions_match(d, p, 0.8, dim=144), np.float32(0.8) * np.float32(0.8))


def other_context_reuse(kind):
    cls, sets, port, ratio = _other_sets(kind)
    ctx = cls(0)
    try:
        for descs in sets:
            pairs = matching.exhaustive_pairs_array(len(descs))
            ctx.set_regions(descs)
            _, off, ij = ctx.run(pairs, ratio)
            fresh = cls(0)
            try:
                fresh.set_regions(descs)
                _, f_off, f_ij = fresh.run(pairs, ratio)
            finally:
                fresh.close()
            o_off, o_ij = port(descs, pairs)
            assert np.array_equal(off, f_off) and np.array_equal(ij, f_ij)
            assert np.array_equal(off, o_off) and np.array_equal(ij, o_ij)
    finally:
        ctx.close()


def cascade_context_reuse():
    from tests.test_cascade import load
    descs, xy, hs, bs, pairs, ref = load("synthetic")
    n = len(descs)
    perm = list(range(n))[::-1]
    sets = [list(range(n)), list(range(n // 2 + 1)), perm, list(range(n))]   # all images -> fewer -> reversed order -> all again
    ctx = matching.CascadeContext(0)
    try:
        for sel in sets:
            d, h, b = [descs[k] for k in sel], [hs[k] for k in sel], [bs[k] for k in sel]
            p = matching.exhaustive_pairs_array(len(sel))
            ctx.set_regions(d, h, b)
            _, off, ij = ctx.run(p, np.float32(0.8) * np.float32(0.8))
            got = _oracle.offsets_to_dict(p, off, ij)
            fresh = matching.CascadeContext(0)
            try:
                fresh.set_regions(d, h, b)
                _, f_off, f_ij = fresh.run(p, np.float32(0.8) * np.float32(0.8))
            finally:
                fresh.close()
            assert np.array_equal(off, f_off) and np.array_equal(ij, f_ij)
            want = {}
            for I, J in p:
                if len(d[I]) and len(d[J]):
                    m = _oracle.port_cascade_match_pair(d[I], h[I], b[I], d[J], h[J], b[J], 0.8)
                    if len(m):
                        want[(int(I), int(J))] = m
            _same(got, want)
    finally:
        ctx.close()


def test_match_context_reuse_emulated():
    with _emu.emulated():
        match_context_reuse()


@pytest.mark.parametrize("kind", ["hamming", "l2f", "l2u8"])
def test_other_context_reuse_emulated(kind):
    with _emu.emulated():
        other_context_reuse(kind)


def test_cascade_context_reuse_emulated():
    with _emu.emulated():
        cascade_context_reuse()
