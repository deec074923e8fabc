"""bench.py --dump-outputs without the hardware: the --rehearsal path (the HIP emulation libraries in place of libmvgx_hip.so, a tiny
image set) writes what its last timed pass delivered, and that is the lists of the CPU restatement, streamed or collected alike."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--rehearsal", "--no-ba",
           "--no-cpu-baseline", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    files = sorted(os.listdir(out_dir))
    assert files == ["match_counts.npy", "sample_matches.npy", "stats.npy"], files
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) < 64 << 20
    out = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


@pytest.mark.skipif(not os.path.isdir(os.path.join(ROOT, "tests", "native", "hipemu")), reason="HIP emulation sources absent")
def test_bench_dump_outputs_are_the_oracle_lists(tmp_path):
    from openmvg_amd import matching, synth
    streamed = _dump(tmp_path / "streamed")
    collected = _dump(tmp_path / "collected", "--collect")
    for name in streamed:
        assert np.array_equal(streamed[name], collected[name]), name

    # the rehearsal's inputs (bench.py: 10 images x 96 descriptors, the bench seed, ratio 0.8): every pair is counted and listed
    descs = synth.image_descriptors(10, n_desc=96, seed=0xC0FFEE00)
    pairs = matching.exhaustive_pairs_array(10)
    offsets, ij = _oracle.port_matcher_regions_match(descs, pairs, 0.8)
    counts = np.diff(offsets.astype(np.int64))
    assert np.array_equal(streamed["match_counts"], np.column_stack([pairs, counts]).astype(np.float64))
    rows = np.column_stack([np.repeat(pairs, counts, axis=0), ij]).astype(np.float64)
    assert rows.shape[0] > 0 and np.array_equal(streamed["sample_matches"], rows)
    assert np.array_equal(streamed["stats"], [len(pairs), 45 * 96 * 96, rows.shape[0]])
