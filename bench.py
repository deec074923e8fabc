#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X matching + BA hot path (contract: see the driver's prompt).

  python bench.py --gpus N --steps K --warmup W            the headline leg alone: set up, warm up, time K steps, print the line
  python bench.py --gpus N --steps K --warmup W --full     ... and every side record and check after the same timed steps

One "step" = one pass of the matching hot path over this rank's shard of the exhaustive pair list (+ one BA LM
iteration on the BA scene when the BA kernels are built). Workloads (BASELINE.json):
  N = 1     configs[1]: 1k images x 2k SIFT (499 500 image pairs = 2.0e12 descriptor pairs) on one MI355X
  N = 2, 4  the same set, pair list cut into N contiguous shards ("scaling": "strong")
  N = 8     configs[3]: 10k images x 2k SIFT (49 995 000 image pairs = 2.0e14 descriptor pairs), pair-sharded x8
Descriptors are replicated, no data-path collective. The BA side record is configs[2] at N = 1 (plus configs[4] on one GPU)
and configs[4] itself, point-sharded over the N ranks with the RCCL exchange, at N > 1.

`value` = descriptor pairs (distance evaluations) per second over all ranks, inputs resident in HBM when the clock
starts, result lists delivered to host memory inside the timed region (streamed batch by batch through two pinned buffers
per rank - mvgx_match_run_stream - so the host footprint does not depend on the size of the run).

A plain run stops there: its line carries the headline fields, the workload and the roofline figures the timed steps' own kernel
timers give. --full adds what takes runs of its own - the CPU reference beside the device with the sampled parity check, the N > 1
self-check, the BA scenes, the Hamming / float / 144-byte matchers, the Matcher_Regions::Match boundary, the geometric filters and
guided matching - and writes the full records to the side file; the timed steps and the headline are the same in both forms.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# ONE peak constant for the i8 matrix pipe (DESIGN.md section 6 cites the same): 1 024 SIMDs x 1 024 MAC/clk x 2 x 2.4 GHz = 5.03 POPS,
# i.e. 2x the 2.5 PF bf16 dense figure of MI355X_MICROARCH.md (its own i8 microbenchmark floor is ">= 3 944 TOPS"). Measured here on
# zero operands, profiles/round1_ubench_valu_mfma_call3.log: 4 759 TOPS with v_mfma_i32_32x32x32_i8, 4 986 with 16x16x64.
I8_MFMA_DENSE_PEAK_TFLOPS = 5000.0
I8_PEAK_NOTE = ("nominal: 1024 SIMDs x 1024 MAC/clk x 2 x 2.4 GHz = 2x the 2.5 PF bf16 dense figure (MI355X_MICROARCH.md; its i8 microbenchmark floor: "
                ">= 3944 TOPS); tools/ubench.hip on zero operands: 4759 TOPS (32x32x32), 4986 (16x16x64), profiles/round1_ubench_valu_mfma_call3.log")
FLOP_PER_DESC_PAIR = 256.0          # 128 MAC
# HBM bytes of the filter kernel per image pair (2000 x 2000 descriptors): the PMC pass of one pass over THIS workload on this
# round's tree, committed under profiles/ (tools/pmc_traffic_summary.py: (TCC_EA0_RDREQ x 64 B x 2 [gfx950 correction for 16 B/lane
# streams, MI355X_MICROARCH.md] + TCC_EA0_WRREQ x 64 B) / 499 500 pairs). Counters cannot be read inside this process; the
# figure is scaled to this run's pairs per launch and the record names the file it came from. Algorithmic minimum (every image
# read once) is ~0.1 GB per launch.
MATCH_TRAFFIC_PROFILES = ("profiles/round6_match_traffic_pmc.json", "profiles/round5_match_traffic_pmc.json", "profiles/round4_match_traffic_pmc.json", "profiles/round2_match_traffic_pmc_call26.json")


def match_traffic_profile():
    for rel in MATCH_TRAFFIC_PROFILES:
        try:
            with open(os.path.join(ROOT, rel)) as f:
                return float(json.load(f)["filter_kernel"]["bytes_per_image_pair"]), rel
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=0, help="images at N=1 (default 1000 = configs[1])")
    ap.add_argument("--desc", type=int, default=2000)
    ap.add_argument("--variant", type=int, default=-1)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--batch-pairs", type=int, default=0, help="image pairs per device batch (default: library default)")
    ap.add_argument("--overlap", type=int, default=-1, help="0: one batch at a time (isolated kernel timings); default: library default (1)")
    ap.add_argument("--verify-alone", type=int, default=-1, help="1: a filter kernel never shares the device with the previous batch's verify kernel; default: library default")
    ap.add_argument("--filter-shape", type=int, default=0, help="MFMA shape of the filter kernel: 16 (v_mfma_i32_16x16x64_i8, library default), 17 (the same with three workgroups per CU: l2_filter16h_kernel) or 32 (A/B runs)")
    ap.add_argument("--collect", action="store_true", help="keep the run's match lists in one pinned host buffer (mvgx_match_run) "
                                                           "instead of streaming them (default)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything else: the CPU baseline and the parity of a sample, "
                         "the N > 1 self-check, the BA, Hamming, float / 144-byte L2, adapter-boundary, geometric-filter and guided-matching "
                         "records (each can still be switched off by its --no-... option); without it only the headline leg runs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--parity-seconds", type=float, default=2.0, help="N > 1: seconds of CPU matching per rank for the sampled parity check")
    ap.add_argument("--no-ba", action="store_true")
    ap.add_argument("--no-selfcheck", action="store_true", help="N > 1: skip tools/scale_selfcheck.py (sharded vs one-device agreement, both BA transports)")
    ap.add_argument("--side-deadline", type=float, default=900.0, help="seconds granted to the side records (BA, Hamming, float L2)")
    ap.add_argument("--no-hamming", action="store_true", help="skip the BRUTE_FORCE_HAMMING side record (N=1 only)")
    ap.add_argument("--no-ba-c5", action="store_true", help="skip the single-GPU run of BASELINE.json configs[4] (1k cams / 5M obs)")
    ap.add_argument("--side-stdout", action="store_true", help="also print the full side records on earlier `SIDE <name> <json>` stdout lines "
                                                               "(default: only gpurun_out/bench_side.json; the LAST stdout line is always the compact driver line)")
    ap.add_argument("--rehearsal", action="store_true",
                    help="TEST HOOK (tests/test_bench_rehearsal_cpu.py), never a measurement: the N > 1 control flow of this file on a box "
                         "without GPUs - gloo process group, the HIP emulation libraries of tests/native (the same device source compiled "
                         "for the host) in place of libmvgx_hip.so, the BA exchange through the callback transport over gloo, a tiny image "
                         "set and BA scene. The printed line carries \"rehearsal\": true.")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller (rank 0's shard) as DIR/<name>.npy: "
                         "see OutputDump")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:   # a plain run is the headline leg alone: every side leg is one of these switches
        args.no_cpu_baseline = args.no_selfcheck = args.no_ba = args.no_ba_c5 = args.no_hamming = True
    return args


class OutputDump:
    """--dump-outputs: the match lists the last timed pass delivered, captured batch by batch from the same pass (streamed) or read
    from the context after it (--collect), written as float64 .npy files, < 64 MB in all:
      match_counts.npy    (K, 3)  [I, J, number of matches] for every image pair, or a fixed seeded sample of 2^20 pairs if more
      sample_matches.npy  (M, 4)  [I, J, i, j] the full lists of a fixed seeded sample of up to 1024 pairs (in pair order, cut at 32 MB)
      stats.npy           (3,)    [image pairs, descriptor pairs, matches] of the pass
    The descriptors and pair lists are seeded, so the same arguments give the same inputs on every run and build."""
    SEED = 0x5EED0D
    MAX_COUNT_PAIRS = 1 << 20
    LIST_PAIRS = 1024
    LIST_BYTES = 32 << 20

    def __init__(self, pairs):
        self.pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(self.pairs)
        rng = np.random.default_rng(self.SEED)
        self.count_idx = np.arange(n) if n <= self.MAX_COUNT_PAIRS else np.sort(rng.choice(n, self.MAX_COUNT_PAIRS, replace=False))
        self.counts = np.full(len(self.count_idx), -1, np.int64)   # -1: a pair the pass never delivered
        self.list_idx = np.sort(rng.choice(n, min(n, self.LIST_PAIRS), replace=False))
        self.lists = {}

    def on_batch(self, p0, off, ij):
        """Lists of pairs [p0, p0 + len(off) - 1): offsets relative to the batch's ij. Cheap: a few hundred slices per pass."""
        p1 = p0 + len(off) - 1
        lo, hi = np.searchsorted(self.count_idx, [p0, p1])
        k = self.count_idx[lo:hi] - p0
        self.counts[lo:hi] = off[k + 1].astype(np.int64) - off[k].astype(np.int64)
        lo, hi = np.searchsorted(self.list_idx, [p0, p1])
        for p in self.list_idx[lo:hi]:
            self.lists[int(p)] = np.array(ij[int(off[p - p0]):int(off[p - p0 + 1])])
        return False   # (a true value would stop the run)

    def write(self, out_dir, st):
        os.makedirs(out_dir, exist_ok=True)
        counts = np.concatenate([self.pairs[self.count_idx], self.counts[:, None]], axis=1).astype(np.float64)
        rows, nbytes = [], 0
        for p in self.list_idx:
            m = self.lists.get(int(p), np.zeros((0, 2), np.uint32))
            nbytes += m.shape[0] * 4 * 8
            if nbytes > self.LIST_BYTES:
                break
            rows.append(np.concatenate([np.broadcast_to(self.pairs[p], (m.shape[0], 2)), m.astype(np.int64)], axis=1))
        sample = np.concatenate(rows).astype(np.float64) if rows else np.zeros((0, 4))
        stats = np.array([st.n_pairs, st.n_desc_pairs, st.n_matches], np.float64)
        for name, a in (("match_counts", counts), ("sample_matches", sample), ("stats", stats)):
            np.save(os.path.join(out_dir, name + ".npy"), a)


def cpu_baseline(descs, pairs, ratio, budget_s):
    """Reference CPU path (oracle/_ref: openMVG's own Matcher_Regions, -O3 -mavx2 OpenMP/std::async build) — or the C
    restatement if the reference build is absent — timed on a bounded random sample of the same pair list."""
    from tests import _oracle
    rng = np.random.default_rng(123)
    kind = "reference" if _oracle.have_ref_match() else "port"
    fn = _oracle.ref_matcher_regions_match if kind == "reference" else _oracle.port_matcher_regions_match
    order = rng.permutation(len(pairs))
    fn(descs, pairs[order[:8]], ratio)   # first call: thread pool / page-in, not timed
    t0 = time.perf_counter()
    fn(descs, pairs[order[8:40]], ratio)
    per_pair = max((time.perf_counter() - t0) / 32.0, 1e-5)
    n = int(max(32, min(len(pairs), budget_s / per_pair)))   # sized for ~budget_s seconds of host work
    sample = pairs[order[:n]]
    dp = float(sum(len(descs[a]) * len(descs[b]) for a, b in sample))
    t0 = time.perf_counter()
    lists = fn(descs, sample, ratio)
    dt = time.perf_counter() - t0
    if kind == "port":   # (offsets, ij) -> {(I, J): (n, 2)} like the reference shim returns
        lists = _oracle.offsets_to_dict(sample, *lists)
    cores = os.cpu_count() or 1
    if kind == "port":
        cores = _oracle.port().oracle_num_threads()
    return {"value": dp / dt, "unit": "descriptor pairs/s", "cores": int(cores), "kind": kind,
            "sample": f"{n} random image pairs of the same set ({dp:.3g} descriptor pairs) in {dt:.1f} s"}, sample, lists


def parity_on_sample(ctx, ratio_sq, sample, cpu_lists):
    """"bit-exact comparison is done on the sampled pairs" - the device lists of the very pairs the CPU baseline
    just matched (same context, same resident descriptors as the timed region) against the CPU lists, entry by entry."""
    from tests import _oracle
    _, offsets, ij = ctx.run(sample, ratio_sq, fetch=True)
    gpu = _oracle.offsets_to_dict(sample, offsets, ij)
    same = set(gpu) == set(cpu_lists) and all(np.array_equal(gpu[k], cpu_lists[k]) for k in gpu)
    return {"pairs_checked": int(len(sample)), "non_empty_pairs": int(len(cpu_lists)),
            "matches_checked": int(sum(len(v) for v in cpu_lists.values())), "identical": bool(same),
            "against": "cpu_baseline lists (same run, same pairs)"}


def adapter_match_boundary_record(descs, n_images, n_desc, ratio, reps=3):
    """Matcher_Regions::Match(regions_provider, exhaustive pairs, container) through the replacement TU
    (openmvg_amd/adapter/mvgx_matcher_regions.cpp in the test harness library, called the way main_ComputeMatches calls it:
    oracle/ref_shim_match.cpp is the CALLER here, not the thing measured): wall time of the whole call, container filled.
    The first call of a process pays what a process pays once (HIP start, code objects, page-locked buffers, fresh heap pages for
    ~1 GB of lists); the later ones are what a host that matches repeatedly sees. pairs/s = descriptor pairs of the call / its wall time."""
    import ctypes as C
    from tests import _oracle
    if not os.path.exists(_oracle.ADAPTER_SO):
        return {"status": "adapter harness library not built (needs the openMVG tree at build time)"}
    lib = C.CDLL(_oracle.ADAPTER_SO, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    arrs, ptrs, cnt = _oracle._desc_tables(descs)
    lib.ref_matcher_regions_match_u8_timed.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_float, C.c_void_p]
    ctr = (C.c_uint64 * 3)()
    lib.mvgx_adapter_counters(ctr, 1)
    calls = []
    for _ in range(reps):
        o = np.zeros(3)
        lib.ref_matcher_regions_match_u8_timed(ptrs, cnt, n_images, C.c_float(ratio), o.ctypes.data)
        calls.append({"match_s": float(o[0]), "matches": int(o[1]), "non_empty_pairs": int(o[2])})
    lib.mvgx_adapter_counters(ctr, 0)
    n_pairs = n_images * (n_images - 1) // 2
    desc_pairs = float(sum(int(cnt[i]) * int(cnt[j]) for i in range(n_images) for j in range(i + 1, n_images))) if n_images <= 64 else float(n_pairs) * n_desc * n_desc
    best = min(c["match_s"] for c in calls[1:]) if len(calls) > 1 else calls[0]["match_s"]
    if hasattr(lib, "mvgx_adapter_match_release_context"):
        lib.mvgx_adapter_match_release_context()
    return {"metric": "descriptor pairs/s at the Matcher_Regions::Match boundary (replacement TU, container filled)",
            "workload": f"{n_images} images x {n_desc}, {n_pairs} image pairs", "calls": calls,
            "first_call_s": calls[0]["match_s"], "repeated_call_s": best,
            "value": desc_pairs / best, "value_first_call": desc_pairs / calls[0]["match_s"], "unit": "descriptor pairs/s",
            "device_pairs": int(ctr[0]) // reps, "fallback_pairs": int(ctr[1]), "device_failures": int(ctr[2]),
            "note": "first_call_s includes the one-time costs of this process' first stream run through the adapter (page-locked result buffers, "
                    "fresh heap pages for the lists); HIP itself was already started by the headline leg"}


def emit(out, args):
    """Full record -> gpurun_out/bench_side.json (+ `SIDE` lines on request); stdout ENDS with the one compact driver line (< 4 KB,
    bench_line.py). fd 2 is flushed first and nothing is written after the line."""
    import bench_line
    side_rel = os.path.join("gpurun_out", "bench_side.json")
    try:
        if not args.full:   # a plain run has no side records: the line is all of it, and a --full run's file stays as it is
            side_rel = None
        elif getattr(args, "rehearsal", False):
            # (the CPU test of the control flow must not replace the measurement the last GPU run left in gpurun_out/ - VERDICT r5 item 7)
            import tempfile
            fd, side_rel = tempfile.mkstemp(prefix="mvgx_bench_rehearsal_side_", suffix=".json")
            with os.fdopen(fd, "w") as f:
                json.dump(out, f)
        else:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, side_rel), "w") as f:
                json.dump(out, f)
    except OSError:
        side_rel = None
    if args.side_stdout:
        for k, v in out.items():
            if isinstance(v, dict) and k not in ("config", "roofline", "cpu_baseline", "parity"):
                print("SIDE " + k + " " + json.dumps(v), flush=True)
    _, line = bench_line.compact(out, side_rel)
    sys.stderr.flush()
    sys.stdout.write(line + "\n")
    sys.stdout.flush()


class quiet_stderr:
    """fd 2 -> gpurun_out/bench_stderr.log while the reference's code runs (its logger writes `INFO: [Matcher_Regions.cpp:41] ...` and
    Ceres reports to stderr; on the driver's capture that chatter followed - and displaced - the bench line of round 4). Python-level
    tracebacks of this process still reach the real stderr: the redirection is undone on exit of the block."""
    saved = None

    def __enter__(self):
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            self.log = open(os.path.join(ROOT, "gpurun_out", "bench_stderr.log"), "ab")
            sys.stderr.flush()
            self.saved = os.dup(2)
            os.dup2(self.log.fileno(), 2)
        except OSError:
            self.saved = None
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            sys.stderr.flush()
            os.dup2(self.saved, 2)
            os.close(self.saved)
            self.log.close()
        return False


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch
    import torch.distributed as dist
    rehearsal = args.rehearsal
    if rehearsal:
        # the emulation libraries are test infrastructure (tests/_emu.py): only this flag routes the C ABI to them
        from tests import _emu
        globals()['_emulation'] = _emu.emulated()   # (kept alive: the context manager restores the real library when collected)
        globals()['_emulation'].__enter__()
        local_rank = 0
        if world > 1:
            dist.init_process_group(backend="gloo")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (no CPU fallback)")
        torch.cuda.set_device(local_rank)
        if world > 1:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    tdev = "cpu" if rehearsal else "cuda"

    from openmvg_amd import matching, synth

    n_images = args.images if args.images > 0 else (10 if rehearsal else 10000 if world >= 8 else 1000)
    if rehearsal:
        args.desc = min(args.desc, 96)
    descs = synth.image_descriptors(n_images, n_desc=args.desc, seed=0xC0FFEE00)
    all_pairs = matching.exhaustive_pairs_array(n_images)
    from openmvg_amd import sharding
    pairs = np.ascontiguousarray(sharding.shard_pairs(all_pairs, [len(d) for d in descs], rank, world))

    selfcheck = None
    if world > 1 and not args.no_selfcheck:
        # multi-GPU readiness (tools/scale_selfcheck.py): rank 0 runs the in-process sharded forms of both halves over all visible
        # devices against the one-device run before anything is timed; the other ranks wait at the barrier
        if rank == 0:
            import subprocess
            try:
                env = dict(os.environ, MVGX_SELFCHECK_REHEARSAL="1") if rehearsal else None
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scale_selfcheck.py")], capture_output=True, text=True, timeout=600, env=env)
                selfcheck = json.loads(r.stdout.strip().splitlines()[-1]) if r.stdout.strip() else {"ok": False, "error": r.stderr[-400:]}
            except Exception as e:
                selfcheck = {"ok": False, "error": repr(e)}
        # (the other ranks wait on the host: a barrier of the RCCL group would park a spinning kernel on every other GPU while the
        # self-check - its own process - uses those GPUs, and would run into the group's collective timeout if the check is slow)
        try:
            wait_group = dist.new_group(backend="gloo")
            dist.barrier(group=wait_group)
        except Exception:
            dist.barrier()

    ctx = matching.MatchContext(local_rank)
    if args.variant >= 0:
        ctx.set_option("variant", args.variant)
    if args.filter_shape:
        ctx.set_option("filter_shape", args.filter_shape)
    if args.overlap >= 0:
        ctx.set_option("overlap", args.overlap)
    if args.verify_alone >= 0:
        ctx.set_option("verify_alone", args.verify_alone)
    if args.batch_pairs > 0:
        ctx.set_option("batch_pairs", args.batch_pairs)
    elif rehearsal:
        ctx.set_option("batch_pairs", 8)   # several batches through the two-slot pipeline
    elif len(pairs) < 16 * 32768:   # a shard of the 1k-image set: keep >= 16 batches in the two-slot pipeline (fill / drain)
        ctx.set_option("batch_pairs", max(4096, len(pairs) // 16))
    ctx.set_option("profile", 1)
    ctx.set_regions(descs)  # descriptors resident in HBM (tile layout built here, outside the timed region)
    ratio_sq = np.float32(args.ratio) * np.float32(args.ratio)

    def barrier():
        if world > 1:
            dist.barrier()
        if not rehearsal:
            torch.cuda.synchronize()

    def one_pass(on_batch=None):
        if args.collect:
            return ctx.run(pairs, ratio_sq, fetch=False)[0]
        return ctx.run_stream(pairs, ratio_sq, on_batch)      # every batch's lists reach host memory; nothing is kept

    for _ in range(args.warmup):
        one_pass()

    dump = OutputDump(pairs) if args.dump_outputs and rank == 0 else None
    kernel_ms = 0.0
    launches = 0
    desc_pairs = 0
    matches = 0
    barrier()
    t0 = time.perf_counter()
    for step in range(args.steps):
        st = one_pass(dump.on_batch if dump is not None and step == args.steps - 1 else None)
        kernel_ms += st.kernel_ms
        launches += int(st.n_kernel_launches)
        desc_pairs += int(st.n_desc_pairs)
        matches = int(st.n_matches)
        variant = int(st.variant)
    barrier()
    dt = time.perf_counter() - t0
    if dump is not None:
        if args.collect:
            dump.on_batch(0, *ctx.results(len(pairs)))
        dump.write(args.dump_outputs, st)

    if world > 1:
        t = torch.tensor([dt, float(desc_pairs), kernel_ms, float(launches)], dtype=torch.float64, device=tdev)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone()
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt = float(tmax[0])
        total_desc_pairs = float(tsum[1])
    else:
        total_desc_pairs = float(desc_pairs)

    if rank == 0:
        value = total_desc_pairs / dt
        # roofline of the dominant kernel (l2_top2_ratio), this rank: algorithmic flop per launch / mean launch time
        flop_per_launch = (desc_pairs / max(launches, 1)) * FLOP_PER_DESC_PAIR
        mean_launch_s = (kernel_ms / max(launches, 1)) * 1e-3
        achieved = flop_per_launch / mean_launch_s / 1e12 if mean_launch_s > 0 else 0.0
        bytes_per_pair, traffic_file = match_traffic_profile()
        out = {
            "metric": "descriptor pairs/s (brute-force L2 2-NN + ratio matching)",
            "value": value,
            "unit": "descriptor pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak" if world >= 8 or world == 1 else "strong",
            "vs_baseline": None,
            "dtype": "i8 (int32 accumulate)",
            "data": "synthetic",
            **({"rehearsal": True} if rehearsal else {}),
            "config": {"workload": f"{n_images} images x {args.desc} SIFT-like uint8x128 descriptors, exhaustive pairs "
                                   f"({len(all_pairs)} image pairs, {len(pairs)} on rank 0), ratio {args.ratio}",
                       "kernel_variant": variant, "matches_rank0": matches,
                       "results": "collected (one pinned host buffer)" if args.collect else "streamed (two pinned batch buffers)",
                       "parallelism": f"pair-sharded x{world}, no collective"},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": I8_MFMA_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / I8_MFMA_DENSE_PEAK_TFLOPS, "peak_note": I8_PEAK_NOTE,
                         "traffic": (bytes_per_pair * (args.desc / 2000.0) * len(pairs) * args.steps / max(launches, 1)
                                     if variant == 4 and bytes_per_pair else None),
                         "traffic_source": f"{traffic_file} (a rocprofv3 --pmc pass of this command, scaled by pairs per launch: "
                                           "counters cannot be read inside this process)",
                         "kernel": ({32: "l2_filter_kernel", 17: "l2_filter16h_kernel"}.get(args.filter_shape, "l2_filter16_kernel")) if variant == 4 else "l2_top2_ratio_kernel",
                         "launches": launches,
                         "mean_launch_ms": kernel_ms / max(launches, 1)},
        }
        if selfcheck is not None:
            out["scale_selfcheck"] = selfcheck
        if world == 1 and not args.no_cpu_baseline:
            try:
                with quiet_stderr():
                    out["cpu_baseline"], sample, cpu_lists = cpu_baseline(descs, all_pairs, args.ratio, args.cpu_seconds)
                    out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
                    out["parity"] = parity_on_sample(ctx, ratio_sq, sample, cpu_lists)
            except Exception as e:  # the baseline is a reported side figure; never let it kill the bench line
                out["cpu_baseline"] = {"value": None, "unit": "descriptor pairs/s", "cores": os.cpu_count(),
                                       "kind": "port", "sample": f"failed: {e!r}"}
    if world > 1 and not args.no_cpu_baseline:
        # N > 1: no CPU throughput figure (rank 0 at N = 1 only), but correctness evidence for EVERY rank's shard: each rank in
        # turn (the host cores are shared) matches a small random sample of ITS pairs on the CPU and compares its device lists
        # entry by entry; the verdicts are combined over the ranks.
        par = None
        for turn in range(world):
            if turn == rank:
                try:
                    _, sample, cpu_lists = cpu_baseline(descs, pairs, args.ratio, args.parity_seconds)
                    par = parity_on_sample(ctx, ratio_sq, sample, cpu_lists)
                except Exception as e:
                    par = {"pairs_checked": 0, "non_empty_pairs": 0, "matches_checked": 0, "identical": False, "error": repr(e)}
            dist.barrier()
        t = torch.tensor([float(par["pairs_checked"]), float(par["non_empty_pairs"]), float(par["matches_checked"]),
                          0.0 if par["identical"] else 1.0], dtype=torch.float64, device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        if rank == 0:
            out["parity"] = {"pairs_checked": int(t[0]), "non_empty_pairs": int(t[1]), "matches_checked": int(t[2]),
                             "identical": bool(t[3] == 0.0), "ranks_checked": world, "ranks_differing": int(t[3]),
                             "against": "the reference's CPU path on a random sample of every rank's own pair shard (same run)"}
    ctx.close()
    ba_rec = ba_c5 = None
    # The side records below must never cost the headline line: if one of them stalls (the BA leg has collectives; a rank
    # that fails alone would leave the others waiting), every rank gives up after a deadline and rank 0 prints what it has.
    import threading

    def give_up():
        if rank == 0:
            out.setdefault("ba", {"status": f"no result within {args.side_deadline:.0f} s"})
            emit(out, args)
        os._exit(0)

    watchdog = threading.Timer(args.side_deadline, give_up)
    watchdog.daemon = True
    watchdog.start()
    quiet = quiet_stderr()   # the side legs run the reference beside the device: its stderr logging goes to gpurun_out/bench_stderr.log
    if args.full:
        quiet.__enter__()
    if not args.no_ba:   # every rank takes part (the BA leg has a real exchange step); rank 0 reports
        try:
            from bench_ba import ba_bench_record
            ba_rec = ba_bench_record(local_rank, world, cpu=not args.no_cpu_baseline, rehearsal=rehearsal)
            if world == 1 and not args.no_ba_c5 and not rehearsal:   # configs[4] fits one GPU: reported beside its sharded runs at N > 1
                ba_c5 = ba_bench_record(local_rank, 1, cpu=not args.no_cpu_baseline, name="c5")
                try:   # C3's size with a realistic track-length distribution (side record; the reference beside it on a short budget)
                    out["ba_mixed_track_lengths"] = ba_bench_record(local_rank, 1, cpu=not args.no_cpu_baseline, cpu_budget_s=30.0, name="mixed")
                except Exception as e:
                    out["ba_mixed_track_lengths"] = {"status": f"failed: {e!r}"}
        except Exception as e:  # the BA leg is a side record: never lose the matching line
            ba_rec = ba_rec or {"status": f"failed: {e!r}"}
    if rank == 0 and world == 1 and not args.no_hamming and not rehearsal:
        try:
            from bench_hamming import hamming_bench_record, l2f_bench_record
            out["hamming"] = hamming_bench_record(local_rank, cpu=not args.no_cpu_baseline)
            out["l2_float"] = l2f_bench_record(local_rank, cpu=not args.no_cpu_baseline)
            from bench_hamming import l2u8_bench_record
            out["l2_uint8_144"] = l2u8_bench_record(local_rank, cpu=not args.no_cpu_baseline)
        except Exception as e:  # side record only
            out["hamming"] = {"status": f"failed: {e!r}"}
        try:   # what the drop-in caller sees: Matcher_Regions::Match through the replacement TU, same workload
            out["adapter_match_boundary"] = adapter_match_boundary_record(descs, n_images, args.desc, args.ratio)
        except Exception as e:
            out["adapter_match_boundary"] = {"status": f"failed: {e!r}"}
        try:   # the step after putative matching
            from bench_geofilter import geofilter_bench_record
            out["geometric_filter"] = geofilter_bench_record(local_rank, cpu=not args.no_cpu_baseline)
            out["geometric_filter_homography"] = geofilter_bench_record(local_rank, n_pairs=20000, cpu=not args.no_cpu_baseline, cpu_pairs=3000, model="h")
            out["geometric_filter_essential"] = geofilter_bench_record(local_rank, n_pairs=20000, steps=1, cpu=not args.no_cpu_baseline, cpu_pairs=3000, model="e")
        except Exception as e:
            out["geometric_filter"] = {"status": f"failed: {e!r}"}
        try:   # the geometric filters' second stage (guided matching)
            from bench_geofilter import guided_matching_bench_record
            out["guided_matching"] = guided_matching_bench_record(local_rank, cpu=not args.no_cpu_baseline)
        except Exception as e:
            out["guided_matching"] = {"status": f"failed: {e!r}"}
        try:   # the other -g models of main_GeometricFilter (angular essential a / u, orthographic essential o): one pass each
            from bench_geofilter import geofilter_other_models_record
            out["geometric_filter_other_models"] = geofilter_other_models_record(local_rank, cpu=not args.no_cpu_baseline)
        except Exception as e:
            out["geometric_filter_other_models"] = {"status": f"failed: {e!r}"}
    if rank == 0:
        if ba_rec is not None:
            out["ba"] = ba_rec
        if ba_c5 is not None:
            out["ba_c5_single_gpu"] = ba_c5
    watchdog.cancel()
    quiet.__exit__(None, None, None)
    if rank == 0:
        emit(out, args)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
