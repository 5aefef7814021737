"""Times the chain tracks -> landmarks -> bundle adjustment on 1024 windows of 5 poses x 2000 slots, two routes in
the same process, alternating:

  host    what the library offered before rank 10: tracks and `seen` as orbx_lk_windows_fetch leaves them on the
          host; per window the landmarks as orbx::build_landmarks makes them (one orbx_triangulate round trip in
          camera 0's frame, the move to the world frame, the depth check and the compaction on the host); then ONE
          orbx_bundle_adjust_batch over all windows.  The assembly is vectorised numpy, so some of this route's time
          is Python's.
  device  tracks and `seen` on the device (as orbx_lk_windows_results_device leaves them):
          orbx_landmarks_build_device + orbx_bundle_adjust_landmarks_device + the fetch of poses and summaries.

Both end with poses and summaries on the host; a host clock runs around each.  The scenes are those of
tests/landmarks_ref.py (sigma = 0.3 px, 10 % outliers on the later frames, tracks of 2-5 frames, poses 2 .. perturbed);
--distinct of them are generated and repeated to fill the batch.  The two routes triangulate differently (camera 0's
frame through float against the world frame in binary64), so their landmark counts and iteration counts are printed
side by side.  After a warm-up of each route: best and median of --reps.

  python tools/landmarks_probe.py [--windows 1024] [--slots 2000] [--reps 10] [--route both|host|device]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--poses", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route", choices=("both", "host", "device"), default="both")
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import landmarks_ref as R

    pkg = __graft_entry__.load_package()
    K = np.ascontiguousarray(R.K_KITTI)
    W = a.poses
    scenes = [R.make_scene(900 + i, W=W, slots=a.slots, sigma=0.3, outliers=0.1, min_seen=2, pose_pert=0.002)
              for i in range(min(a.distinct, a.windows))]
    pick = [scenes[i % len(scenes)] for i in range(a.windows)]
    poses, tracks, seen = R.stack(pick)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = (pkg.orbx.BaSummary * a.windows)()
    rot = [[R.rodrigues(p[:3]) for p in sc["poses"][:2]] for sc in scenes]
    with pkg.Context(pkg.default_params("gpu")) as c:
        f = c._lib.orbx_bundle_adjust_batch
        d_tracks, d_seen = torch.from_numpy(tracks).cuda(), torch.from_numpy(seen).cuda()
        torch.cuda.synchronize()
        split = {}

        def host_route():
            t0 = time.perf_counter()
            pts, op, oq, xy, npts, nobs = [], [], [], [], [0], [0]
            for w in range(a.windows):
                R0, R1 = rot[w % len(scenes)]
                p, t, s = poses[w], tracks[w], seen[w]
                Rr = R1 @ R0.T
                tr = p[1, 3:] - Rr @ p[0, 3:]
                tri = np.flatnonzero(s >= 2)
                xyz, valid = c.triangulate(t[tri, 0], t[tri, 1], K, Rr, tr)
                X = (xyz.astype(np.float64) - p[0, 3:]) @ R0  # R0^T (x - t0)
                keep = tri[(valid != 0) & (X[:, 2] > 0)]
                live = np.arange(W)[None, :] < s[keep][:, None]
                pts.append(X[(valid != 0) & (X[:, 2] > 0)])
                op.append(np.repeat(np.arange(len(keep), dtype=np.int32), s[keep]))
                oq.append(np.nonzero(live)[1].astype(np.int32))
                xy.append(t[keep][live].astype(np.float64))
                npts.append(npts[-1] + len(keep))
                nobs.append(nobs[-1] + len(op[-1]))
            P = np.ascontiguousarray(poses.reshape(-1, 6).copy())
            X, xy = np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.concatenate(xy))
            op, oq = np.concatenate(op), np.concatenate(oq)
            po = (np.arange(a.windows + 1) * W).astype(np.int32)
            xo, oo = np.int32(npts), np.int32(nobs)
            t1 = time.perf_counter()
            st = f(c._h, K.ctypes.data_as(DP), a.windows, po.ctypes.data_as(IP), P.ctypes.data_as(DP),
                   xo.ctypes.data_as(IP), X.ctypes.data_as(DP), oo.ctypes.data_as(IP), op.ctypes.data_as(IP),
                   oq.ctypes.data_as(IP), xy.ctypes.data_as(DP), 1.0, 200, out)
            t2 = time.perf_counter()
            c._chk(st)
            split["host"] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
            return (t2 - t0) * 1e3, int(npts[-1]), [s.iterations for s in out], [s.termination for s in out]

        def device_route():
            t0 = time.perf_counter()
            c.landmarks_build(K, d_tracks, d_seen, poses)
            c.bundle_adjust_landmarks(1.0, 200)
            t1 = time.perf_counter()
            _, sums, _ = c.bundle_adjust_landmarks_fetch(points=False)
            t2 = time.perf_counter()
            split["device"] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
            return (t2 - t0) * 1e3, 0, [s["iterations"] for s in sums], [s["termination"] for s in sums]

        routes = {"host": host_route, "device": device_route}
        names = [a.route] if a.route != "both" else ["host", "device"]
        for n in names:  # warm-up: the buffers grow on the first call
            routes[n]()
        ms = {n: [] for n in names}
        last = {}
        for _ in range(a.reps):
            for n in names:
                t, npt, its, term = routes[n]()
                ms[n].append(t)
                last[n] = (its, term, split[n], npt)
        v = c.landmarks_view() if "device" in names else None
        res = {"windows": a.windows, "poses": W, "slots": a.slots, "reps": a.reps}
        if v is not None:
            tot = c.landmarks_fetch()
            res["device_landmarks"] = int(tot["point_offset"][-1])
            res["device_observations"] = int(tot["obs_offset"][-1])
        for n in names:
            its, term, sp, npt = last[n]
            keys = ("build_on_host", "bundle_adjust_batch") if n == "host" else ("enqueue", "wait_and_fetch")
            res[n] = {"ms_best": min(ms[n]), "ms_median": float(np.median(ms[n])), "ms_all": [round(x, 2) for x in ms[n]],
                      "last_split_ms": {keys[0]: round(sp[0], 2), keys[1]: round(sp[1], 2)},
                      "iters_mean": float(np.mean(its)), "iters_max": int(np.max(its)),
                      "terminations": [int(np.sum(np.array(term) == k)) for k in range(4)]}
            if n == "host":
                res[n]["landmarks"] = npt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
