"""ctypes view of the sequential restatement tests/cpp/lm_views_sequential.cpp, beside
tests/landmarks_seq.py, whose compile_so builds it (test infrastructure; not part of build())."""
import ctypes as C

import numpy as np

from landmarks_seq import KEYS

FIRST_TWO, WIDEST, ALL_VIEWS = range(3)
KEPT, SHORT, DEGENERATE, BEHIND, REPROJECTION, NO_WINDOW = range(6)
MODES = (FIRST_TWO, WIDEST, ALL_VIEWS)


def seq_views_build(lib, K, poses, tracks, seen, tri_mode, max_reproj_px, pose_status=None):
    """A batch through seq_lm_views_build: (block in the format of Context.landmarks_fetch, reason (n, slots) uint8,
    reproj_px (n, slots) float32).  poses (n, W, 6), tracks (n, slots, W, 2) float32, seen (n, slots) int32."""
    K = np.ascontiguousarray(K, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    tracks = np.ascontiguousarray(tracks, np.float32)
    seen = np.ascontiguousarray(seen, np.int32)
    n, cap, W = tracks.shape[:3]
    assert poses.shape == (n, W, 6) and seen.shape == (n, cap)
    out = dict(status=np.zeros(n, np.int32), point_offset=np.zeros(n + 1, np.int32),
               obs_offset=np.zeros(n + 1, np.int32), points3=np.zeros((n * cap, 3)),
               slot_of_point=np.zeros(n * cap, np.int32), obs_point=np.zeros(n * cap * W, np.int32),
               obs_pose=np.zeros(n * cap * W, np.int32), obs_xy=np.zeros((n * cap * W, 2)))
    reason, px = np.zeros((n, cap), np.uint8), np.zeros((n, cap), np.float32)
    ps = None if pose_status is None else np.ascontiguousarray(pose_status, np.int32)
    lib.seq_lm_views_build.restype = None
    lib.seq_lm_views_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + \
        [C.c_int, C.c_double] + [C.c_void_p] * 3
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    lib.seq_lm_views_build(p(K), n, cap, W, p(poses), p(tracks), p(seen), *[p(out[k]) for k in KEYS], tri_mode,
                           float(max_reproj_px), p(ps), p(reason), p(px))
    N, M = int(out["point_offset"][n]), int(out["obs_offset"][n])
    for k in ("points3", "slot_of_point"):
        out[k] = out[k][:N].copy()
    for k in ("obs_point", "obs_pose", "obs_xy"):
        out[k] = out[k][:M].copy()
    out["pose_offset"] = (np.arange(n + 1) * W).astype(np.int32)
    return out, reason, px
