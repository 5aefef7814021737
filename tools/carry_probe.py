"""Measures the landmarks carry on many streams at once: --streams independent camera
paths (tests/carry_ref.py's make_stream: no noise, float32 pixels), each cut into three generations of windows of
--frames frames that share one frame, --slots slots per window of which a fifth ends inside the window and is replaced
by fresh points in the next.  Composed from the step entries:

  generation 0    tracks pose -> chain -> chained landmarks -> PnP of frames >= 2 -> seeded solve
  generation g    carry (the solved points) -> carried PnP of every frame -> carried build [-> solve]

A window's length ratio is |c_last - c_first| of the window over |c_1 - c_0| of the stream's generation 0, against
the same ratio of the true path; counted: the windows of each generation whose ratio is more than 1e-3 off.  Beside
it, the same streams one by one through orbx_stream_odometry_tracks_device with scale alignment, which needs two
shared frames: windows of the same length at stride frames - 2 over the same frames (each tracking the stream's first
--slots points through all its frames), and the same measure on the same frames of the stitched trajectory.

A host clock runs around one generation (carry, carried PnP, carried build: enqueue, then a wait through a one-window
fetch) after a warm-up: best and median of --reps.  Kernel times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/carry_probe.py --reps 3 --stitch-streams 0

  python tools/carry_probe.py [--streams 1024] [--frames 5] [--slots 200] [--reps 10] [--stitch-streams N]
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


def centres(poses6):
    """camera centres (..., 3) of world -> camera (angle-axis, t) poses (..., 6)"""
    import landmarks_ref as LR

    flat = poses6.reshape(-1, 6)
    return np.array([-LR.rodrigues(p[:3]).T @ p[3:] for p in flat]).reshape(poses6.shape[:-1] + (3,))


def ratio_off(c_window, c_gen0, t_window, t_gen0):
    """|c_last - c_first| / |c_1 - c_0 of generation 0| against the true path, relative: one value per stream"""
    dist = lambda c: np.linalg.norm(c[:, -1] - c[:, 0], axis=1)
    unit = lambda c: np.linalg.norm(c[:, 1] - c[:, 0], axis=1)
    with np.errstate(all="ignore"):
        return np.abs((dist(c_window) / unit(c_gen0)) / (dist(t_window) / unit(t_gen0)) - 1.0)


def summary(off):
    return {"above_1e-3": int((~(off <= 1e-3)).sum()), "share_above_1e-3": float((~(off <= 1e-3)).mean()),
            "max": float(np.nanmax(off)), "median": float(np.nanmedian(off))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--slots", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stitch-streams", type=int, default=-1, help="streams sent through the stitch (-1: all)")
    ap.add_argument("--threshold-px", type=float, default=2.0)
    ap.add_argument("--max-iters", type=int, default=1000)
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import carry_ref as R

    pkg = __graft_entry__.load_package()
    VO, P, CY, ST = pkg.orbx_vo, pkg.orbx_pnp, pkg.orbx_carry, pkg.orbx_stream
    n, L, G = a.streams, a.frames, 3
    K = np.ascontiguousarray(R.K)
    pnp_args = dict(prob=0.99, threshold_px=a.threshold_px, max_iters=a.max_iters, seed=0, refine_iters=10,
                    min_inliers=6)
    stride = L - 2  # of the stitched route
    n_st = -(-(G * (L - 1) + 1 - L) // stride) + 1  # windows that cover the generations' frames
    streams = []
    wins = R.scale_streams(n, L, a.slots, G, a.slots // 5, seed=5000,
                           extra_frames=(n_st - 1) * stride + L - (G * (L - 1) + 1), streams=streams)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tracks = [dev(np.stack([w["tracks"] for w in wins[g]])) for g in range(G)]
    seen = [dev(np.stack([w["seen"] for w in wins[g]])) for g in range(G)]
    origin = [None] + [dev(np.stack([w["origin"] for w in wins[g]])) for g in range(1, G)]
    torch.cuda.synchronize()
    true_c = [centres(np.stack([w["true_poses"] for w in wins[g]])) for g in range(G)]
    res = {"streams": n, "frames": L, "slots": a.slots, "generations": G, "pnp_args": pnp_args, "reps": a.reps}

    with pkg.Context(pkg.default_params("gpu")) as c:
        def generation0():
            c.tracks_pose(K, tracks[0], seen[0])
            VO.window_poses(c)
            VO.landmarks_build_chained(c, K, tracks[0], seen[0])
            P.window_poses_pnp(c, **pnp_args)
            P.bundle_adjust_landmarks_pnp(c)

        def generation(g, source):
            CY.landmarks_carry(c, origin[g], source=source)
            CY.window_poses_pnp_carried(c, K, tracks[g], seen[g], **pnp_args)
            CY.landmarks_build_carried(c, K, tracks[g], seen[g])

        for name, source, solve in (("solved", CY.CARRY_SOLVED, True), ("built", CY.CARRY_BUILT, False)):
            ms, first = [], None
            for rep in range(a.reps + 1):  # the first repetition grows the buffers
                generation0()
                c0 = centres(c.bundle_adjust_landmarks_fetch(points=False)[0] if solve
                             else P.window_poses_pnp_fetch(c, masks=False)["poses6"])
                out = {}
                for g in range(1, G):
                    c.landmarks_fetch(0, 1)  # (nothing of the earlier stages is left in flight)
                    t0 = time.perf_counter()
                    generation(g, source)
                    t1 = time.perf_counter()
                    c.landmarks_fetch(0, 1)
                    ms.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
                    if solve:
                        c.bundle_adjust_landmarks()
                    got = CY.window_poses_pnp_carried_fetch(c, masks=False)
                    rec = got["records"]
                    out["generation_%d" % g] = {
                        "length_ratio_off": summary(ratio_off(centres(got["poses6"]), c0, true_c[g], true_c[0])),
                        "windows_lost": int((got["window_status"] != CY.CARRY_OK).sum()),
                        "pnp_status_counts": {str(k): int((rec["status"] == k).sum()) for k in np.unique(rec["status"])},
                        "n_corr_median": float(np.median(rec["n_corr"])), "iters_median": float(np.median(rec["iters"])),
                        "carried_median": float(np.median(CY.landmarks_carry_fetch(c)["count"])),
                        "landmarks_ok": int((c.landmarks_fetch()["status"] == 0).sum())}
                if first is None:
                    first = out
                else:
                    assert json.dumps(out) == json.dumps(first), "a repetition gave other results"
            total = [t for t, _ in ms[2:]]
            first.update({"generation_call_ms_best": min(total), "generation_call_ms_median": float(np.median(total)),
                          "generation_call_ms_all": [round(t, 3) for t in total],
                          "generation_enqueue_ms_median": float(np.median([e for _, e in ms[2:]]))})
            res["carry_" + name] = first

        # the same streams through the stitch, one stream per call
        m = n if a.stitch_streams < 0 else min(n, a.stitch_streams)
        if m > 0:
            off = {g: np.zeros(m) for g in range(1, G)}
            bad = 0
            for i in range(m):
                own = [R.window(streams[i], w * stride, L, np.arange(a.slots), np.full(a.slots, L)) for w in range(n_st)]
                tr, se = np.stack([w["tracks"] for w in own]), np.stack([w["seen"] for w in own])
                ST.stream_odometry_tracks_device(c, K, tr, se, stride=stride, align_scale=True)
                st = ST.stitch_fetch(c)
                bad += int((st["status"] != 0).any())
                cen = st["trajectory4x4"][:, :3, 3]
                for g in range(1, G):
                    f = g * (L - 1)
                    off[g][i] = ratio_off(cen[None, f:f + L], cen[None, :L], true_c[g][i:i + 1], true_c[0][i:i + 1])[0]
            res["stitched"] = {"streams": m, "windows": n_st, "stride": stride, "streams_with_a_window_not_ok": bad,
                               **{"generation_%d" % g: {"length_ratio_off": summary(off[g])} for g in range(1, G)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
