"""State kept between calls on the MI355X: the call sequence and the library-level re-use of tests/test_adapter_kept_context_cpu.py
against libmvgx_hip.so, at the full sizes, plus the switch from device-resident regions to host regions on one MatchContext."""
import numpy as np
import pytest

from openmvg_amd import matching, synth
from tests import _oracle
from tests.test_adapter_kept_context_cpu import (cascade_context_reuse, kept_context_sequence, match_context_reuse,
                                                 other_context_reuse)

pytestmark = pytest.mark.gpu


def test_kept_context_sequence_on_the_device(monkeypatch):
    """the sequence on the adapter library. B: 30 images x 700 rows. C: 9 000 / 34 000 / 1 rows - 34 000 rows put more than 16 384
    rows in one norm-parity class, so the batch of the adapter's default 16 384 pairs shrinks under mvgx_match_run's scratch cap"""
    if not _oracle.have_adapter():
        pytest.skip("adapter library not built (needs the openMVG tree)")
    kept_context_sequence(_oracle.adapter(), monkeypatch, (30, 700, [9000, 34000, 1]))


def test_match_context_reuse_on_the_device():
    match_context_reuse()


@pytest.mark.parametrize("kind", ["hamming", "l2f", "l2u8"])
def test_other_context_reuse_on_the_device(kind):
    other_context_reuse(kind)


def test_cascade_context_reuse_on_the_device():
    cascade_context_reuse()


def test_device_regions_then_host_regions_on_one_context():
    """set_regions_device (rows owned by the caller) and then set_regions (rows owned by the context) on one MatchContext, and back:
    each run equals the restatement on its own image set"""
    import ctypes as C
    from openmvg_amd import _capi
    _capi.lib()
    # the HIP runtime libmvgx_hip.so was loaded with (whatever its soname): opening the mapped file again returns the same handle
    with open("/proc/self/maps") as maps:
        runtime = sorted({ln.split()[-1] for ln in maps if "/libamdhip64.so" in ln})
    assert runtime, "libmvgx_hip.so loaded no HIP runtime"
    hip = C.CDLL(runtime[0])
    first = synth.image_descriptors(6, n_desc=400, seed=21)
    first[2] = first[2][:0]
    second = synth.image_descriptors(9, n_desc=520, seed=22)
    second[4] = second[4][:3]
    r2 = np.float32(0.8) * np.float32(0.8)

    def check(descs, off, ij):
        pairs = matching.exhaustive_pairs_array(len(descs))
        o_off, o_ij = _oracle.port_matcher_regions_match(descs, pairs, 0.8)
        assert np.array_equal(off, o_off) and np.array_equal(ij, o_ij) and int(o_off[-1]) > 0

    host = np.ascontiguousarray(np.concatenate(first))
    d_first = C.c_void_p()
    assert hip.hipSetDevice(0) == 0 and hip.hipMalloc(C.byref(d_first), C.c_size_t(host.nbytes)) == 0
    assert hip.hipMemcpy(d_first, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0   # hipMemcpyHostToDevice
    ctx = matching.MatchContext(0)
    try:
        ctx.set_regions_device(d_first.value, [len(d) for d in first])
        _, off, ij = ctx.run(matching.exhaustive_pairs_array(len(first)), r2)
        check(first, off, ij)
        ctx.set_regions(second)
        _, off, ij = ctx.run(matching.exhaustive_pairs_array(len(second)), r2)
        check(second, off, ij)
        ctx.set_regions_device(d_first.value, [len(d) for d in first])
        _, off, ij = ctx.run(matching.exhaustive_pairs_array(len(first)), r2)
        check(first, off, ij)
    finally:
        ctx.close()
        hip.hipFree(d_first)
