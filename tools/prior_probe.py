"""Measures landmark priors in the window solve on tools/carry_probe.py's streams:
--streams independent camera paths (tests/carry_ref.py's make_stream: no noise, float32 pixels), three generations of
windows of --frames frames that share one frame, --slots slots per window of which a fifth ends inside the window.

  generation 0    tracks pose -> chain -> chained landmarks -> PnP of frames >= 2 -> seeded solve
  generation g    carry -> carried PnP of every frame -> carried build [-> priors of the carried landmarks] [-> solve]

in four variants: `solved` (the plain solve behind every carried build, the solved points carried on), `built` (no
solve, the built points carried on) -- the two rows of profiles/landmarks_carry/ --, and `prior_given` / `prior_anchor`
(orbx_landmarks_priors_carried_device with --weight, then orbx_bundle_adjust_landmarks_prior_device from the built
points or from the anchors, the solved points carried on), the last two again at --weight x 100.  The measure is
carry_probe's: a window's length ratio |c_last - c_first| over |c_1 - c_0| of the stream's generation 0 against the
true path's, read from the carried PnP's poses; counted: the windows more than 1e-3 off.  Beside it, how far the
anchored landmarks end from their anchors.

A host clock runs around one generation of the `prior_anchor` variant (carry, carried PnP, carried build, priors and
solve enqueued, then a wait through a one-window fetch) after a warm-up: best and median of --reps.  Kernel times come
from a trace run of its own, in which --compare-solves runs the plain and the prior solve on the same blocks in turn:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prior_probe.py --reps 3 --compare-solves

  python tools/prior_probe.py [--streams 1024] [--frames 5] [--slots 200] [--reps 10] [--weight 1.0] [--compare-solves]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--slots", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weight", type=float, default=1.0)
    ap.add_argument("--threshold-px", type=float, default=2.0)
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--compare-solves", action="store_true",
                    help="only: the plain and the prior solve in turn on the same blocks, for a kernel trace")
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import carry_ref as R
    from carry_probe import centres, ratio_off, summary

    pkg = __graft_entry__.load_package()
    VO, P, CY, PR = pkg.orbx_vo, pkg.orbx_pnp, pkg.orbx_carry, pkg.orbx_prior
    n, L, G = a.streams, a.frames, 3
    K = np.ascontiguousarray(R.K)
    pnp_args = dict(prob=0.99, threshold_px=a.threshold_px, max_iters=a.max_iters, seed=0, refine_iters=10,
                    min_inliers=6)
    # (carry_probe's streams to the frame: it draws the frames its stitched route needs behind the last generation,
    # and the stream's random path depends on how many frames are drawn)
    stride = L - 2
    n_st = -(-(G * (L - 1) + 1 - L) // stride) + 1
    wins = R.scale_streams(n, L, a.slots, G, a.slots // 5, seed=5000,
                           extra_frames=(n_st - 1) * stride + L - (G * (L - 1) + 1))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tracks = [dev(np.stack([w["tracks"] for w in wins[g]])) for g in range(G)]
    seen = [dev(np.stack([w["seen"] for w in wins[g]])) for g in range(G)]
    origin = [None] + [dev(np.stack([w["origin"] for w in wins[g]])) for g in range(1, G)]
    torch.cuda.synchronize()
    true_c = [centres(np.stack([w["true_poses"] for w in wins[g]])) for g in range(G)]
    res = {"streams": n, "frames": L, "slots": a.slots, "generations": G, "pnp_args": pnp_args, "reps": a.reps,
           "weight": a.weight}

    with pkg.Context(pkg.default_params("gpu")) as c:
        def generation0():
            c.tracks_pose(K, tracks[0], seen[0])
            VO.window_poses(c)
            VO.landmarks_build_chained(c, K, tracks[0], seen[0])
            P.window_poses_pnp(c, **pnp_args)
            P.bundle_adjust_landmarks_pnp(c)

        def generation(g, source, weight=None, start=None, solve=True):
            CY.landmarks_carry(c, origin[g], source=source)
            CY.window_poses_pnp_carried(c, K, tracks[g], seen[g], **pnp_args)
            CY.landmarks_build_carried(c, K, tracks[g], seen[g])
            if weight is not None:
                PR.landmarks_priors_carried(c, weight)
                PR.bundle_adjust_landmarks_prior(c, start=start)
            elif solve:
                c.bundle_adjust_landmarks()

        if a.compare_solves:
            generation0()
            for rep in range(a.reps + 1):
                for g in range(1, G):
                    generation(g, CY.CARRY_SOLVED, solve=False)
                    PR.landmarks_priors_carried(c, a.weight)
                    c.bundle_adjust_landmarks()                                  # k_ba_lm<false>
                    PR.bundle_adjust_landmarks_prior(c, start=PR.PRIOR_START_GIVEN)   # k_ba_lm<true>, the same start
                    PR.bundle_adjust_landmarks_prior(c, start=PR.PRIOR_START_ANCHOR)  # k_ba_lm<true>, from the anchors
                    c.landmarks_fetch(0, 1)
            res["compare_solves"] = {"plain_solves": 2 * (a.reps + 1), "prior_solves": 4 * (a.reps + 1),
                                     "order_per_generation": ["plain", "prior_given", "prior_anchor"]}
            print(json.dumps(res))
            return

        variants = [("solved", CY.CARRY_SOLVED, None, None, True), ("built", CY.CARRY_BUILT, None, None, False)]
        for wt in (a.weight, a.weight * 100.0):
            variants += [("prior_given_w%g" % wt, CY.CARRY_SOLVED, wt, PR.PRIOR_START_GIVEN, True),
                         ("prior_anchor_w%g" % wt, CY.CARRY_SOLVED, wt, PR.PRIOR_START_ANCHOR, True)]
        timed = "prior_anchor_w%g" % a.weight
        for name, source, weight, start, solve in variants:
            reps = a.reps if name == timed else 1
            ms, first = [], None
            for rep in range(reps + 1):  # the first repetition grows the buffers
                generation0()
                c0 = centres(c.bundle_adjust_landmarks_fetch(points=False)[0] if solve
                             else P.window_poses_pnp_fetch(c, masks=False)["poses6"])
                out = {}
                for g in range(1, G):
                    c.landmarks_fetch(0, 1)  # (nothing of the earlier stages is left in flight)
                    t0 = time.perf_counter()
                    generation(g, source, weight, start, solve)
                    t1 = time.perf_counter()
                    c.landmarks_fetch(0, 1)
                    ms.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
                    got = CY.window_poses_pnp_carried_fetch(c, masks=False)
                    row = {"length_ratio_off": summary(ratio_off(centres(got["poses6"]), c0, true_c[g], true_c[0])),
                           "windows_lost": int((got["window_status"] != CY.CARRY_OK).sum())}
                    if solve:
                        _, ss, sx = c.bundle_adjust_landmarks_fetch()
                        term = np.array([s["termination"] for s in ss])
                        row["terminations"] = {str(k): int((term == k).sum()) for k in np.unique(term)}
                        row["iterations_median"] = float(np.median([s["iterations"] for s in ss]))
                        row["iterations_max"] = int(max(s["iterations"] for s in ss))
                    if weight is not None:
                        pri = PR.landmarks_priors_fetch(c)
                        on = pri["prior_weight"] > 0
                        move = np.linalg.norm(sx[on] - pri["prior_xyz"][on], axis=1) / np.linalg.norm(pri["prior_xyz"][on], axis=1)
                        row["anchored_landmarks"] = int(on.sum())
                        row["anchored_median_per_window"] = float(np.median(pri["count"]))
                        row["anchor_move_relative"] = {"max": float(move.max()), "median": float(np.median(move))}
                    out["generation_%d" % g] = row
                if first is None:
                    first = out
                else:
                    assert json.dumps(out) == json.dumps(first), "a repetition gave other results"
            if name == timed:
                total = [t for t, _ in ms[2:]]
                first.update({"generation_call_ms_best": min(total), "generation_call_ms_median": float(np.median(total)),
                              "generation_call_ms_all": [round(t, 3) for t in total],
                              "generation_enqueue_ms_median": float(np.median([e for _, e in ms[2:]]))})
            res[name] = first
    print(json.dumps(res))


if __name__ == "__main__":
    main()
