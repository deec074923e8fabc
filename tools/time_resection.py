"""Times mvgx_resection_localize on the MI355X: 1 / 16 / 256 problems of 100 / 1 000 / 10 000 correspondences, 30 % outliers.

  python tools/time_resection.py [--repeat 3] [--solver ding] [--max-iteration 4096] [--error-max PX] [--uncalibrated] [--digest]

--error-max PX (finite): the bounded form, mvgx_resection_localize_bounded, on the same problems.
--uncalibrated: mvgx_resection_localize_uncalibrated (the six-point DLT loop of a view without intrinsics) on the same problems, the
image size 1280 x 960 in place of the intrinsics. With --max-iteration 1 every problem runs one solve, one sort and one NFA scan: the
fixed part that the solver's share of the kernel time is read against (models / iterations of the full run are printed for it).
--digest: every line also carries a sha256 over what the last call returned - ok, pose, P (and K of the uncalibrated entry), error_max,
min_nfa and the inlier list of every problem: two builds of the library that print the same digests computed the same bits.

Prints one JSON line per (problems, correspondences): kernel_ms = HIP events around the prepare pass and the a-contrario kernels
(mvgx_resection_stats), total_ms = the whole call with uploads, downloads, KRt_From_P on the host; medians over --repeat calls after one
warm-up call; iterations = a-contrario iterations run over all problems. Needs a GPU: there is no CPU path."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openmvg_amd import _capi, resection   # noqa: E402


def make_problems(n_problems, n, outliers=0.3, noise=0.5, seed=0x5E):
    """pinhole views (f = 1000, 1280 x 960) of points 4 .. 9 units in front of a random pose; a share of the pixels replaced by uniform ones"""
    rng = np.random.default_rng(seed)
    from scipy.spatial.transform import Rotation
    x2d, X3d, poses = [], [], []
    for _ in range(n_problems):
        R = Rotation.from_rotvec(rng.normal(size=3) * 0.3).as_matrix()
        t = rng.normal(size=3) * 0.5 + (0.0, 0.0, 6.0)
        pc = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.0, 2.0, n), rng.uniform(4.0, 9.0, n)], 1)
        x = np.stack([640.0 + 1000.0 * pc[:, 0] / pc[:, 2], 480.0 + 1000.0 * pc[:, 1] / pc[:, 2]], 1) + rng.normal(size=(n, 2)) * noise
        bad = rng.permutation(n)[: int(round(outliers * n))]
        x[bad] = np.stack([rng.uniform(0, 1280, len(bad)), rng.uniform(0, 960, len(bad))], 1)
        x2d.append(x); X3d.append((pc - t) @ R); poses.append((R, t))
    intr = np.zeros((n_problems, 8))
    intr[:, :3] = (1000.0, 640.0, 480.0)
    return (np.arange(n_problems + 1, dtype=np.uint64) * n, np.concatenate(x2d), np.concatenate(X3d), np.ones(n_problems, np.int32), intr), poses


def digest(out):
    """sha256 over the outputs of one call (a list of resection.Localization), problem by problem"""
    h = hashlib.sha256()
    for o in out:
        h.update(bytes([int(o.ok)]))
        for a in (o.R, o.t, o.C, o.P, getattr(o, "K", None), o.error_max, o.min_nfa):
            if a is not None:
                h.update(np.ascontiguousarray(a, np.float64).tobytes())
        h.update(np.ascontiguousarray(o.inliers, np.uint32).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--solver", default="ding")
    ap.add_argument("--max-iteration", type=int, default=4096)
    ap.add_argument("--error-max", type=float, default=float("inf"), help="a finite bound in pixels times the bounded form")
    ap.add_argument("--uncalibrated", action="store_true", help="times mvgx_resection_localize_uncalibrated (six-point DLT, no intrinsics)")
    ap.add_argument("--digest", action="store_true", help="adds a sha256 over the last call's outputs to every line")
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--sizes", type=int, nargs="*", default=[100, 1000, 10000])
    a = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("time_resection.py needs a GPU")
    for n in a.sizes:
        for n_problems in a.problems:
            args, poses = make_problems(n_problems, n)
            kw = dict(solver=a.solver, max_iteration=a.max_iteration)
            bounded = np.isfinite(a.error_max)
            run = (lambda *p, **k: resection.localize_bounded(*p, a.error_max, **k)) if bounded else resection.localize
            if a.uncalibrated:
                if bounded:
                    raise SystemExit("the six-point loop has no bounded form")
                args = args[:3] + ([(1280, 960)] * n_problems,)
                kw = dict(max_iteration=a.max_iteration)
                run = resection.localize_uncalibrated
            run(*args, **kw)   # warm-up: code objects, the stream, the slab caches
            kernel, total = [], []
            for _ in range(a.repeat):
                out, st = run(*args, **kw)
                kernel.append(st.kernel_ms); total.append(st.total_ms)
            err = [float(np.abs(o.R - R).max()) for o, (R, _) in zip(out, poses) if o.ok]
            extra = dict(digest=digest(out)) if a.digest else {}
            print(json.dumps(dict(problems=n_problems, correspondences=n, solver="dlt6" if a.uncalibrated else a.solver, max_iteration=a.max_iteration,
                                  error_max=a.error_max if bounded else None, kernel_ms_median=float(np.median(kernel)), kernel_ms_min=float(min(kernel)), kernel_ms_max=float(max(kernel)),
                                  total_ms_median=float(np.median(total)), iterations=int(st.n_iterations), models=int(st.n_models),
                                  ok=int(sum(o.ok for o in out)), largest_rotation_error=max(err) if err else None, **extra)), flush=True)


if __name__ == "__main__":
    main()
