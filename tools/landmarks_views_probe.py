"""The landmarks build from every view of a track beside the build of rank 10, at rank 10's profile shape: 1024
windows of 5 poses x 2000 slots, the scenes of tools/landmarks_probe.py.

One process calls, --reps times each and in this order, orbx_landmarks_build_device and then
orbx_landmarks_build_views_device in each mode (first two, widest, all views) with --gate px (default 3; the first-two
mode also once more without a gate, where it prepares two poses per window only).  Meant to run under
`rocprofv3 --kernel-trace --stats --output-format csv`: the kernel times come from the trace, whose dispatches of
k_lm_views / k_lm_triangulate_views stand in the order of the calls (--summarise <kernel_trace.csv> groups them by it).
Without the profiler the probe still prints one JSON line: per call the landmarks kept, and a host clock around
build + wait (which is mostly launch and synchronisation at this size).

It also records, once and without a verdict, whether better points shorten the solve: the sigma = 0.3, outliers = 0.1,
pose_pert = 0.002 window of the landmark tests (seed 401, 300 slots, tilted world) solved from a first-two block and
from an all-views block gated at 3 px -- iterations, initial and final cost, termination.

  python tools/landmarks_views_probe.py [--windows 1024] [--slots 2000] [--reps 3] [--gate 3.0]
  python tools/landmarks_views_probe.py --summarise <kernel_trace.csv> [--reps 3]
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS = ("plain", "first_two_gate0", "first_two", "widest", "all_views")


def summarise(path, reps):
    """Per call of CALLS: the mean duration in us of its kernels, from the dispatches of the trace in order."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        m = re.search(r"\bk_lm_\w+", r["Kernel_Name"])
        if m:
            dur.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    per = reps + 1  # (one warm-up call each)
    n_views = len(CALLS) - 1
    assert len(dur["k_lm_triangulate"]) >= per and len(dur["k_lm_triangulate_views"]) >= per * n_views, \
        {k: len(v) for k, v in dur.items()}
    out["plain"] = {"k_lm_triangulate_us": [round(x, 1) for x in dur["k_lm_triangulate"][1:per]]}
    for i, call in enumerate(CALLS[1:]):
        sl = slice(i * per + 1, (i + 1) * per)
        out[call] = {"k_lm_views_us": [round(x, 1) for x in dur["k_lm_views"][sl]],
                     "k_lm_triangulate_views_us": [round(x, 1) for x in dur["k_lm_triangulate_views"][sl]]}
    out["all_calls"] = {k: {"n": len(v), "mean_us": round(float(np.mean(v)), 1)} for k, v in dur.items()}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--poses", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gate", type=float, default=3.0)
    ap.add_argument("--summarise")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.reps)
    import torch

    import __graft_entry__
    import landmarks_ref as R

    pkg = __graft_entry__.load_package()
    LM = pkg.orbx_lm
    K = np.ascontiguousarray(R.K_KITTI)
    scenes = [R.make_scene(900 + i, W=a.poses, slots=a.slots, sigma=0.3, outliers=0.1, min_seen=2, pose_pert=0.002)
              for i in range(min(a.distinct, a.windows))]
    poses, tracks, seen = R.stack([scenes[i % len(scenes)] for i in range(a.windows)])
    res = {"windows": a.windows, "poses": a.poses, "slots": a.slots, "reps": a.reps, "gate_px": a.gate, "calls": {}}
    with pkg.Context(pkg.default_params("gpu")) as c:
        d_tracks, d_seen = torch.from_numpy(tracks).cuda(), torch.from_numpy(seen).cuda()
        torch.cuda.synchronize()
        builds = {
            "plain": lambda: c.landmarks_build(K, d_tracks, d_seen, poses),
            "first_two_gate0": lambda: LM.landmarks_build_views(c, K, d_tracks, d_seen, poses, LM.TRI_FIRST_TWO, 0.0),
            "first_two": lambda: LM.landmarks_build_views(c, K, d_tracks, d_seen, poses, LM.TRI_FIRST_TWO, a.gate),
            "widest": lambda: LM.landmarks_build_views(c, K, d_tracks, d_seen, poses, LM.TRI_WIDEST, a.gate),
            "all_views": lambda: LM.landmarks_build_views(c, K, d_tracks, d_seen, poses, LM.TRI_ALL_VIEWS, a.gate),
        }
        for call in CALLS:
            ms = []
            for _ in range(a.reps + 1):  # (the first one is the warm-up: the buffers grow)
                t0 = time.perf_counter()
                builds[call]()
                c._chk(c._lib.orbx_landmarks_fetch(c._h, 0, 1, None, None, None, None, None, None, 0, None, None, None,
                                                   0, None, None))  # (waits for the build, copies two offsets)
                ms.append((time.perf_counter() - t0) * 1e3)
            blk = c.landmarks_view()
            off = np.zeros(a.windows + 1, np.int32)
            c._chk(c._lib.orbx_landmarks_fetch(c._h, 0, a.windows, None, None, off.ctypes.data, None, None, None, 0,
                                               None, None, None, 0, None, None))
            res["calls"][call] = {"landmarks": int(off[-1]), "build_and_wait_ms": [round(x, 3) for x in ms[1:]],
                                  "n_windows": blk.n_windows}
            if call != "plain":
                reason, _ = LM.landmarks_views_fetch(c, 0, min(a.windows, len(scenes)))
                res["calls"][call]["reasons_of_the_distinct_windows"] = np.bincount(reason.ravel(), minlength=6).tolist()
        # whether better points shorten the solve: measured once, no verdict
        sc = R.make_scene(401, W=5, slots=300, min_seen=0, world=R.WORLD_TILTED, sigma=0.3, outliers=0.1,
                          pose_pert=0.002)
        res["solve"] = {}
        for name, mode, gate in (("first_two", LM.TRI_FIRST_TWO, 0.0), ("all_views_3px", LM.TRI_ALL_VIEWS, 3.0)):
            LM.landmarks_build_views(c, K, sc["tracks"][None], sc["seen"][None], sc["poses"][None], mode, gate)
            c.bundle_adjust_landmarks(1.0, 200)
            _, sums, pts = c.bundle_adjust_landmarks_fetch()
            res["solve"][name] = dict(sums[0], landmarks=len(pts))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
