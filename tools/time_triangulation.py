"""Times mvgx_triangulate_tracks on a C5-sized scene (1 000 cameras, 500 000 tracks, 5 M observations) on the MI355X.

  python tools/time_triangulation.py [--cams 1000] [--tracks 500000] [--len 10] [--repeat 5] [--model 1]

Prints one JSON line per mode (blind, robust (3, 3), robust (2, 2)): kernel_ms = HIP events around the prepare pass and the track
kernels (mvgx_triangulate_stats), total_ms = the whole call with uploads, downloads and the host's bucketing; medians over --repeat calls
after one warm-up call. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openmvg_amd import _capi, synth, triangulation   # noqa: E402


def make_scene(n_cams, n_tracks, track_len, model, seed=0xC5):
    """cameras on a ring of radius 5 looking at the origin, points in [-1, 1]^3, every track seen by track_len cameras a quarter turn apart
    in all, pixel noise 0.5, 5 % of the observations displaced by 60 px"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_cams) / n_cams
    C = np.stack([5 * np.cos(ang), 0.3 * rng.standard_normal(n_cams), 5 * np.sin(ang)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 1.0, 0.0])[None], z); x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], axis=1)
    poses = np.concatenate([Rotation.from_matrix(R).as_rotvec(), -np.einsum("nij,nj->ni", R, C)], axis=1)
    intr = np.zeros((1, 8))
    intr[0, :3] = (4000.0, 2000.0, 0.0) if model == synth.CAM_SPHERICAL else (1000.0, 500.0, 500.0)
    if model in (synth.CAM_PINHOLE_RADIAL1, synth.CAM_PINHOLE_RADIAL3, synth.CAM_PINHOLE_BROWN, synth.CAM_PINHOLE_FISHEYE):
        intr[0, 3] = -0.05
    pts = rng.uniform(-1, 1, (n_tracks, 3))
    stride = max(1, n_cams // (4 * track_len))
    first = rng.integers(0, n_cams, n_tracks)
    obs_pose = np.sort((first[:, None] + stride * np.arange(track_len)[None]) % n_cams, axis=1).astype(np.uint32).reshape(-1)
    obs_pt = np.repeat(np.arange(n_tracks), track_len)
    xy = synth.project(model, np.repeat(intr, len(obs_pose), 0), poses[obs_pose], pts[obs_pt]) + 0.5 * rng.standard_normal((len(obs_pose), 2))
    bad = rng.random(len(xy)) < 0.05
    xy[bad] += 60.0 * rng.standard_normal((int(bad.sum()), 2))
    start = (np.arange(n_tracks + 1) * track_len).astype(np.uint64)
    return dict(poses=poses, intrinsics=intr, intr_model=np.array([model], np.int32), track_start=start, obs_pose=obs_pose,
                obs_intr=np.zeros(len(obs_pose), np.uint32), obs_xy=xy, points=pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=1000)
    ap.add_argument("--tracks", type=int, default=500000)
    ap.add_argument("--len", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--model", type=int, default=synth.CAM_PINHOLE)
    a = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("time_triangulation.py needs a GPU")
    sc = make_scene(a.cams, a.tracks, a.len, a.model)
    args = [sc[k] for k in ("poses", "intrinsics", "intr_model", "track_start", "obs_pose", "obs_intr", "obs_xy")]
    for name, kw in (("blind", dict(mode="blind")), ("robust_3_3", dict(mode="robust")),
                     ("robust_2_2", dict(mode="robust", min_required_inliers=2, min_sample_index=2))):
        triangulation.triangulate_tracks(*args, **kw)   # warm-up: code objects, the sample table, the slab caches
        kernel, total = [], []
        for _ in range(a.repeat):
            X, ok, inl, st = triangulation.triangulate_tracks(*args, **kw)
            kernel.append(st.kernel_ms); total.append(st.total_ms)
        err = np.linalg.norm(X[ok] - sc["points"][ok], axis=1)
        print(json.dumps(dict(mode=name, cams=a.cams, tracks=a.tracks, observations=int(len(sc["obs_pose"])), model=a.model,
                              kernel_ms_median=float(np.median(kernel)), kernel_ms_min=float(min(kernel)), kernel_ms_max=float(max(kernel)),
                              total_ms_median=float(np.median(total)), kept=int(ok.sum()), inlier_obs=int(inl.sum()),
                              hypotheses=int(st.n_hypotheses), median_point_error=float(np.median(err)))), flush=True)


if __name__ == "__main__":
    main()
