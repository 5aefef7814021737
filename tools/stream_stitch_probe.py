"""Times tracks -> one trajectory on a stream of overlapping windows, two routes in the same process, alternating
(DESIGN.md §9 rank 16).  Both start from tracks and `seen` on the device and run the tracks pose, the stream's chain,
the landmarks build, the solve and the write-back gate there; they differ in the join:

  host    orbx_bundle_adjust_write_back_fetch of every window's poses, then orbx_stitch_windows on the CPU.
  device  orbx_stream_odometry_tracks_device (the same stages and orbx_stitch_windows_device on the write-back's
          block), and ONE orbx_stitch_fetch of the trajectory at the end.

Both end with the trajectory on the host; a host clock runs around each.  The stream is tests/stitch_ref.py's
scene_stream (one camera path through one scene, no noise).  The routes' trajectories are compared bit for bit.
After a warm-up of each route: best and median of --reps.

--fold-windows W runs, instead, orbx_stitch_windows_device alone on W uploaded windows (stitch_ref.make_stream) --reps
times, for a kernel trace of k_st_links, k_st_fold and k_st_apply at a stream length the scene generator is too slow
for; a host clock around enqueue + wait is reported.

  python tools/stream_stitch_probe.py [--windows 1024] [--frames 5] [--stride 2] [--slots 200] [--reps 10]
  python tools/stream_stitch_probe.py --fold-windows 8192
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
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--slots", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fold-windows", type=int, default=0)
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import stitch_ref as R

    pkg = __graft_entry__.load_package()
    S, VO = pkg.orbx_stream, pkg.orbx_vo
    L, stride = a.frames, a.stride
    with pkg.Context(pkg.default_params("gpu")) as c:
        if a.fold_windows:
            W = a.fold_windows
            cs = R.make_stream(W, L, stride, 1, True)
            poses = torch.from_numpy(cs["poses"]).cuda()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps + 1):  # the first call grows the buffers
                t0 = time.perf_counter()
                S.stitch_windows_device(c, poses, stride, cs["T_start"], True)
                got = S.stitch_fetch(c, 0, 1, 0, 1)
                ms.append((time.perf_counter() - t0) * 1e3)
            got = S.stitch_fetch(c)
            want = S.stitch_windows(cs["poses"], stride, cs["T_start"], True)
            print(json.dumps({"fold_windows": W, "frames": L, "stride": stride, "stream_frames": len(got["owner"]),
                              "reps": a.reps, "ms_best": min(ms[1:]), "ms_median": float(np.median(ms[1:])),
                              "equals_host": all(got[k].tobytes() == want[k].tobytes() for k in got)}))
            return
        n = a.windows
        sc = R.scene_stream(n, L, stride, a.slots, 5)
        K = np.ascontiguousarray(sc["K"])
        d_tracks, d_seen = torch.from_numpy(sc["tracks"]).cuda(), torch.from_numpy(sc["seen"]).cuda()
        torch.cuda.synchronize()
        T0 = np.array(sc["true"][0])
        split = {}

        def host_route():
            t0 = time.perf_counter()
            c.tracks_pose(K, d_tracks, d_seen)
            S.window_poses_stream(c, stride)
            VO.landmarks_build_chained(c, K, d_tracks, d_seen)
            c.bundle_adjust_landmarks()
            VO.bundle_adjust_write_back(c)
            t1 = time.perf_counter()
            p4, _ = VO.bundle_adjust_write_back_fetch(c)
            t2 = time.perf_counter()
            out = S.stitch_windows(p4, stride, T0, True)
            t3 = time.perf_counter()
            split["host"] = {"enqueue": t1 - t0, "wait_and_fetch": t2 - t1, "stitch_on_cpu": t3 - t2}
            return (t3 - t0) * 1e3, out["trajectory4x4"]

        def device_route():
            t0 = time.perf_counter()
            S.stream_odometry_tracks_device(c, K, d_tracks, d_seen, stride=stride, T_start=T0, align_scale=True)
            t1 = time.perf_counter()
            v = S.stitch_view(c)
            traj = np.zeros((v.n_frames, 4, 4))
            c._chk(S.load().orbx_stitch_fetch(c._h, 0, v.n_frames, traj.ctypes.data, None, 0, 0, None, None, None))
            t2 = time.perf_counter()
            split["device"] = {"enqueue": t1 - t0, "wait_and_fetch": t2 - t1}
            return (t2 - t0) * 1e3, traj

        routes = {"host": host_route, "device": device_route}
        for name in routes:  # warm-up: the buffers grow on the first call
            routes[name]()
        ms = {name: [] for name in routes}
        last = {}
        for _ in range(a.reps):
            for name in routes:
                t, traj = routes[name]()
                ms[name].append(t)
                last[name] = (traj, dict(split[name]))
        st = S.stitch_fetch(c)
        err_c, err_a = R.similarity_residual(st["trajectory4x4"], sc["true"])
        # what the stages before the join made of the windows (the join cannot mend a window that went wrong)
        good = c.tracks_pose_fetch()["good"]
        _, sums, _ = c.bundle_adjust_landmarks_fetch(points=False)
        term = np.array([s["termination"] for s in sums])
        upd = VO.bundle_adjust_write_back_fetch(c)[1]
        lm = c.landmarks_fetch()["status"]
        stages = {"pairs_without_a_pose": int((good < 5).sum()),
                  "landmark_status_counts": {str(k): int((lm == k).sum()) for k in np.unique(lm)},
                  "termination_counts": {str(k): int((term == k).sum()) for k in np.unique(term)},
                  "windows_with_a_pose_not_written_back": int((upd[:, 1:] == 0).any(axis=1).sum())}
        # every window against the true path in its own gauge: the rotation of rel(w, k) against the true relative
        # rotation, and the lengths |c_k - c_0| / |c_1 - c_0| against the true ratios (the window's scale is free)
        wb = VO.bundle_adjust_write_back_fetch(c)[0]
        rot_err, len_err = np.zeros(n), np.zeros(n)
        for w in range(n):
            true = sc["true"][w * stride:w * stride + L]
            for k in range(1, L):
                Rw = wb[w, 0, :3, :3].T @ wb[w, k, :3, :3]
                Rt = true[0, :3, :3].T @ true[k, :3, :3]
                rot_err[w] = max(rot_err[w], np.arccos(np.clip((np.trace(Rw.T @ Rt) - 1.0) / 2.0, -1.0, 1.0)))
                rw = np.linalg.norm(wb[w, k, :3, 3] - wb[w, 0, :3, 3]) / np.linalg.norm(wb[w, 1, :3, 3] - wb[w, 0, :3, 3])
                rt = np.linalg.norm(true[k, :3, 3] - true[0, :3, 3]) / np.linalg.norm(true[1, :3, 3] - true[0, :3, 3])
                len_err[w] = max(len_err[w], abs(rw / rt - 1.0))
        stages["windows_off_the_true_path"] = {
            "rotation_above_1e-3_rad": int((rot_err > 1e-3).sum()), "rotation_max_rad": float(rot_err.max()),
            "rotation_median_rad": float(np.median(rot_err)), "length_ratio_above_1e-3": int((len_err > 1e-3).sum()),
            "length_ratio_max": float(len_err.max()), "length_ratio_median": float(np.median(len_err))}
        lam = st["lambda"]
        res = {"windows": n, "frames": L, "stride": stride, "slots": a.slots, "stream_frames": len(st["owner"]),
               "stages": stages, "lambda_min_max": [float(lam.min()), float(lam.max())],
               "reps": a.reps, "status_counts": {str(k): int((st["status"] == k).sum()) for k in np.unique(st["status"])},
               "residual_to_true_path_units": err_c, "residual_to_true_path_rad": err_a,
               "path_length_units": float(np.linalg.norm(np.diff(sc["true"][:, :3, 3], axis=0), axis=1).sum())}
        for name in routes:
            traj, sp = last[name]
            res[name] = {"ms_best": min(ms[name]), "ms_median": float(np.median(ms[name])),
                         "ms_all": [round(x, 2) for x in ms[name]],
                         "last_split_ms": {k: round(v * 1e3, 3) for k, v in sp.items()}}
        res["trajectories_equal"] = last["host"][0].tobytes() == last["device"][0].tobytes()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
