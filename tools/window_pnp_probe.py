"""Asks whether the chain's per-pair scales are what puts windows off the true path: the
stream of tools/stream_stitch_probe.py (tests/stitch_ref.py's scene_stream: one camera path through one scene, no
noise) through two routes that share everything up to the landmarks block,

  tracks pose -> stream chain -> chained landmarks            (once per repetition)
  unseeded    -> orbx_bundle_adjust_landmarks_device     -> write-back -> stitch
  seeded      -> orbx_window_poses_pnp_device -> orbx_bundle_adjust_landmarks_pnp_device -> write-back -> stitch

and counts, for each, the windows whose written-back poses are more than 1e-3 rad or 1e-3 (relative length ratio) off
the true path in the window's own gauge -- the two figures of profiles/stream_stitch/README.md.  Also counted: the
same for the seeded poses themselves (before any solve), the PnP statuses, and the solves' terminations.

A host clock runs around the PnP call alone (enqueue, then a wait through a one-window fetch) after a warm-up: best and
median of --reps.  Kernel times (k_pnp_ransac beside k_pose_ransac of the same call) come from a trace run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/window_pnp_probe.py --reps 3

  python tools/window_pnp_probe.py [--windows 1024] [--frames 5] [--stride 2] [--slots 200] [--reps 10]
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


def off_the_path(poses4x4, true, stride):
    """camera -> world poses (n, L, 4, 4) against the true path, window by window in the window's own gauge: the
    largest rotation error of rel(w, k) and the largest relative error of |c_k - c_0| / |c_1 - c_0|"""
    n, L = poses4x4.shape[:2]
    rot_err, len_err = np.zeros(n), np.zeros(n)
    for w in range(n):
        t = true[w * stride:w * stride + L]
        p = poses4x4[w]
        for k in range(1, L):
            Rw, Rt = p[0, :3, :3].T @ p[k, :3, :3], t[0, :3, :3].T @ t[k, :3, :3]
            rot_err[w] = max(rot_err[w], np.arccos(np.clip((np.trace(Rw.T @ Rt) - 1.0) / 2.0, -1.0, 1.0)))
            rw = np.linalg.norm(p[k, :3, 3] - p[0, :3, 3]) / np.linalg.norm(p[1, :3, 3] - p[0, :3, 3])
            rt = np.linalg.norm(t[k, :3, 3] - t[0, :3, 3]) / np.linalg.norm(t[1, :3, 3] - t[0, :3, 3])
            len_err[w] = max(len_err[w], abs(rw / rt - 1.0))
    with np.errstate(invalid="ignore"):
        return {"rotation_above_1e-3_rad": int((~(rot_err <= 1e-3)).sum()), "rotation_max_rad": float(np.nanmax(rot_err)),
                "rotation_median_rad": float(np.nanmedian(rot_err)),
                "length_ratio_above_1e-3": int((~(len_err <= 1e-3)).sum()), "length_ratio_max": float(np.nanmax(len_err)),
                "length_ratio_median": float(np.nanmedian(len_err))}


def to_4x4(poses6):
    """world -> camera (angle-axis, t) blocks (n, L, 6) as camera -> world 4x4"""
    import landmarks_ref as LR

    out = np.zeros(poses6.shape[:2] + (4, 4))
    for w in range(poses6.shape[0]):
        for k in range(poses6.shape[1]):
            R = LR.rodrigues(poses6[w, k, :3])
            out[w, k, :3, :3], out[w, k, :3, 3], out[w, k, 3, 3] = R.T, -R.T @ poses6[w, k, 3:], 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--slots", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threshold-px", type=float, default=2.0)
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--refine-iters", type=int, default=10)
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import stitch_ref as R

    pkg = __graft_entry__.load_package()
    S, VO, P = pkg.orbx_stream, pkg.orbx_vo, pkg.orbx_pnp
    n, L, stride = a.windows, a.frames, a.stride
    pnp_args = dict(prob=0.99, threshold_px=a.threshold_px, max_iters=a.max_iters, seed=0,
                    refine_iters=a.refine_iters, min_inliers=6)
    with pkg.Context(pkg.default_params("gpu")) as c:
        sc = R.scene_stream(n, L, stride, a.slots, 5)
        K = np.ascontiguousarray(sc["K"])
        d_tracks, d_seen = torch.from_numpy(sc["tracks"]).cuda(), torch.from_numpy(sc["seen"]).cuda()
        torch.cuda.synchronize()
        T0 = np.array(sc["true"][0])

        def block():
            c.tracks_pose(K, d_tracks, d_seen)
            S.window_poses_stream(c, stride)
            VO.landmarks_build_chained(c, K, d_tracks, d_seen)

        def finish():
            VO.bundle_adjust_write_back(c)
            S.stitch_windows_device(c, VO.bundle_adjust_write_back_view(c), stride, T0, True)
            wb, upd = VO.bundle_adjust_write_back_fetch(c)
            st = S.stitch_fetch(c)
            err_c, err_a = R.similarity_residual(st["trajectory4x4"], sc["true"])
            _, sums, _ = c.bundle_adjust_landmarks_fetch(points=False)
            term = np.array([s["termination"] for s in sums])
            return {"windows_off_the_true_path": off_the_path(wb, sc["true"], stride),
                    "termination_counts": {str(k): int((term == k).sum()) for k in np.unique(term)},
                    "windows_with_a_pose_not_written_back": int((upd[:, 1:] == 0).any(axis=1).sum()),
                    "initial_cost_median": float(np.median([s["initial_cost"] for s in sums])),
                    "iterations_total": int(sum(s["iterations"] for s in sums)),
                    "stitched_residual_to_true_path_units": err_c, "stitched_residual_to_true_path_rad": err_a}

        ms, res = [], {}
        for rep in range(a.reps + 1):  # the first repetition grows the buffers
            block()
            c.bundle_adjust_landmarks()
            unseeded = finish()
            c.landmarks_fetch(0, 1)  # (nothing of the block's stages is left in flight)
            t0 = time.perf_counter()
            P.window_poses_pnp(c, **pnp_args)
            t1 = time.perf_counter()
            P.window_poses_pnp_fetch(c, 0, 1, masks=False)
            t2 = time.perf_counter()
            ms.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3))
            P.bundle_adjust_landmarks_pnp(c)
            seeded = finish()
            if rep == 0:
                res["unseeded"], res["seeded"] = unseeded, seeded
            else:
                assert unseeded == res["unseeded"] and seeded == res["seeded"], "a repetition gave other results"
        pnp = P.window_poses_pnp_fetch(c, masks=False)
        rec = pnp["records"]
        ok = rec["status"] == P.OK
        res["pnp"] = {"status_counts": {str(k): int((rec["status"] == k).sum()) for k in np.unique(rec["status"])},
                      "iters_median": float(np.median(rec["iters"])), "iters_max": int(rec["iters"].max()),
                      "n_corr_median": float(np.median(rec["n_corr"])),
                      "inlier_share_median": float(np.median(rec["inliers"][ok] / rec["n_corr"][ok])) if ok.any() else 0.0,
                      "rms_px_median": float(np.median(rec["rms_px"][ok])) if ok.any() else 0.0,
                      "seeded_poses_off_the_true_path": off_the_path(to_4x4(pnp["poses6"]), sc["true"], stride)}
        res["chained_poses_off_the_true_path"] = off_the_path(VO.window_poses_fetch(c)["poses4x4"], sc["true"], stride)
        total = [t for t, _ in ms[1:]]
        res.update({"windows": n, "frames": L, "stride": stride, "slots": a.slots, "problems": int(rec.size),
                    "pnp_args": pnp_args, "reps": a.reps,
                    "pnp_call_ms_best": min(total), "pnp_call_ms_median": float(np.median(total)),
                    "pnp_call_ms_all": [round(t, 3) for t in total],
                    "pnp_enqueue_ms_median": float(np.median([e for _, e in ms[1:]]))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
