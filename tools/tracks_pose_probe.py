"""Times tracks -> per-pair pose, points and scale on windows of 5 frames x 2000 slots, two routes in the same
process, alternating:

  host    what the library offered before rank 11: tracks and `seen` as orbx_lk_windows_fetch leaves them on the
          host; per pair the numpy compaction by `seen`, then one estimate_pose + triangulate (+ estimate_scale on
          the slot-joined lists from pair 1 of a window on), each a synchronous round trip.
  device  tracks and `seen` on the device (as orbx_lk_windows_results_device leaves them): ONE
          orbx_tracks_pose_device + orbx_tracks_pose_fetch of the per-pair results.

Both end with R, t and scale of every pair on the host; a host clock runs around each.  The scenes are those of
tests/landmarks_ref.py (sigma = 0.3 px, 10 % outliers on the later frames, tracks of 2-5 frames); --distinct of them
are generated and repeated to fill the batch.  The routes' scales are compared (they compute the same bits).  After a
warm-up of each route: best and median of --reps.

  python tools/tracks_pose_probe.py [--windows 50] [--slots 2000] [--reps 10] [--route both|host|device]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--route", choices=("both", "host", "device"), default="both")
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import landmarks_ref as R

    pkg = __graft_entry__.load_package()
    K = np.ascontiguousarray(R.K_KITTI)
    L = a.frames
    scenes = [R.make_scene(900 + i, W=L, slots=a.slots, sigma=0.3, outliers=0.1, min_seen=2)
              for i in range(min(a.distinct, a.windows))]
    pick = [scenes[i % len(scenes)] for i in range(a.windows)]
    _, tracks, seen = R.stack(pick)
    pairs = a.windows * (L - 1)
    with pkg.Context(pkg.default_params("gpu")) as c:
        d_tracks, d_seen = torch.from_numpy(tracks).cuda(), torch.from_numpy(seen).cuda()
        torch.cuda.synchronize()
        split = {}

        def host_route():
            t0 = time.perf_counter()
            scale = np.ones(pairs)
            clipped = np.clip(seen, 0, L)
            for w in range(a.windows):
                prev = None
                for k in range(L - 1):
                    slots = np.flatnonzero(clipped[w] >= k + 2)
                    p1, p2 = tracks[w, slots, k], tracks[w, slots, k + 1]
                    r = c.estimate_pose(p1, p2, K, max_iters=a.max_iters)
                    xyz, valid = c.triangulate(p1, p2, K, r["R"], r["t"])
                    if prev is not None:
                        # the join on the slot: this pair's slots are a subset of the previous pair's
                        at = np.searchsorted(prev[0], slots)
                        moved = (prev[1][at].astype(np.float64) @ prev[3].T + prev[4]).astype(np.float32)
                        scale[w * (L - 1) + k], _ = c.estimate_scale(moved, xyz, prev[2][at], valid)
                    prev = (slots, xyz, valid, r["R"], r["t"])
            t1 = time.perf_counter()
            split["host"] = ((t1 - t0) * 1e3, 0.0)
            return (t1 - t0) * 1e3, scale

        def device_route():
            t0 = time.perf_counter()
            c.tracks_pose(K, d_tracks, d_seen, max_iters=a.max_iters)
            t1 = time.perf_counter()
            f = c.tracks_pose_fetch()
            t2 = time.perf_counter()
            split["device"] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
            return (t2 - t0) * 1e3, f["scale"]

        routes = {"host": host_route, "device": device_route}
        names = [a.route] if a.route != "both" else ["host", "device"]
        for n in names:  # warm-up: the buffers grow on the first call
            routes[n]()
        ms = {n: [] for n in names}
        last = {}
        for _ in range(a.reps):
            for n in names:
                t, scale = routes[n]()
                ms[n].append(t)
                last[n] = (scale, split[n])
        res = {"windows": a.windows, "frames": L, "slots": a.slots, "pairs": pairs, "reps": a.reps,
               "max_iters": a.max_iters}
        if "device" in names:
            f = c.tracks_pose_fetch()
            res["correspondences"] = int(f["n"].sum())
            res["iters_mean"] = float(f["iters"].mean())
        for n in names:
            scale, sp = last[n]
            res[n] = {"ms_best": min(ms[n]), "ms_median": float(np.median(ms[n])), "ms_all": [round(x, 2) for x in ms[n]],
                      "scale_mean": float(np.mean(scale))}
            if n == "device":
                res[n]["last_split_ms"] = {"enqueue": round(sp[0], 2), "wait_and_fetch": round(sp[1], 2)}
        if len(names) == 2:
            # the host route moves the previous points in numpy (a fused multiply-add free matrix product is not
            # promised there), so the scales are compared by value
            res["scale_max_abs_diff"] = float(np.max(np.abs(last["host"][0] - last["device"][0])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
