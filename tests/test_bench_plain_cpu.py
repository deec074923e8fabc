"""bench.py without --full is the headline leg alone, and --full puts every side record back - checked without the hardware through
the --rehearsal path (the HIP emulation libraries in place of libmvgx_hip.so, a tiny image set and BA scene), one rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline")
SIDE = ("cpu_baseline", "gpu_over_cpu", "parity", "scale_selfcheck", "ba", "ba_c5_single_gpu", "ba_mixed_tracks", "side",
        "side_records_file")


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--rehearsal", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.rstrip("\n").splitlines()
    assert lines and lines[-1].startswith("{") and len(lines[-1]) < 4096
    return json.loads(lines[-1]), lines


def _check_headline(d):
    for k in HEADLINE:
        assert k in d, k
    assert d["rehearsal"] is True and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["metric"] == "descriptor pairs/s (brute-force L2 2-NN + ratio matching)" and d["unit"] == "descriptor pairs/s"
    assert d["higher_is_better"] is True and d["dtype"] == "i8 (int32 accumulate)"
    # value = the descriptor pairs of one pass over the 45 image pairs / the time of a step
    assert d["value"] > 0 and abs(d["value"] - 45 * 96 * 96 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


@pytest.mark.skipif(not os.path.isdir(os.path.join(ROOT, "tests", "native", "hipemu")), reason="HIP emulation sources absent")
def test_a_plain_run_prints_the_headline_and_nothing_else():
    d, lines = _run()
    _check_headline(d)
    for k in SIDE:
        assert k not in d, k
    assert len(lines) == 1, lines
    # the switches of the side legs change nothing about a plain run, and --side-stdout has no record to print
    d2, lines2 = _run("--no-ba", "--no-cpu-baseline", "--no-hamming", "--side-stdout")
    assert set(d2) == set(d) and len(lines2) == 1


@pytest.mark.skipif(not os.path.isdir(os.path.join(ROOT, "tests", "native", "hipemu")), reason="HIP emulation sources absent")
def test_full_adds_the_side_records_to_the_same_headline():
    d, _ = _run("--full", "--side-deadline", "600")
    _check_headline(d)
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["value"] > 0 and d["gpu_over_cpu"] > 0
    assert d["parity"]["identical"] is True and d["parity"]["pairs_checked"] >= 1
    assert d["ba"]["iterations"] >= 1 and d["ba"]["final_rmse"] < d["ba"]["initial_rmse"]
    side = d["side_records_file"]   # the rehearsal's full record goes to a temporary file of its own
    try:
        full = json.load(open(side))
        assert full["value"] > 0 and "ba" in full and "cpu_baseline" in full
    finally:
        os.remove(side)


def test_the_side_legs_of_bench_are_all_behind_full():
    """Every side leg of main() is gated by one of the --no-... switches, and a run without --full sets them all."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"--full", action="store_true"' in src
    gate = src[src.index("if not args.full:"):]
    gate = gate[:gate.index("\n    return args")]
    for name in ("no_cpu_baseline", "no_selfcheck", "no_ba", "no_hamming"):
        assert f"args.{name} =" in gate, name
