"""openmvg_amd — MI355X (gfx950) accelerators behind two openMVG interfaces.

  matching : brute-force L2 2-NN + Lowe ratio on 128-D uint8 descriptors  (openmvg_amd.matching)
  ba       : Levenberg-Marquardt bundle adjustment                         (openmvg_amd.ba)
  triangulation : blind / robust triangulation of the tracks of a scene    (openmvg_amd.triangulation)
  resection     : robust resection of views (AC-RANSAC over P3P), batched   (openmvg_amd.resection: localize for an unbounded
                  precision, localize_bounded for a finite error_max)
  relative_pose : E to (R, t) by cheirality, and robustRelativePose from putative matches, batched (openmvg_amd.relative_pose:
                  from_essential, robust for pinhole pairs, robust_angular on bearing vectors)
  tracks        : feature tracks from pairwise matches with the reference's track ids (openmvg_amd.tracks: build, and observations
                  for the hand-over to triangulation.triangulate_tracks)

All compute lives in openmvg_amd/lib/libmvgx_hip.so (hand-written HIP, C ABI in include/mvgx.h);
the Python modules only mirror the reference's host interfaces. No CPU fallback exists.
"""
__version__ = "0.1.0"
