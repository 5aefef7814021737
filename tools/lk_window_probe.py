"""Times trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499) at the reference's bundle-adjustment shape,
one-launch path and sequential path side by side.

Frames: stream A (streams.py), 1241 x 376, device-resident; window w covers frames w .. w + 4 (a window per new frame);
2000 point slots per window, filled by good_features_batch(2000, 0.01, 8) on each window's first frame and left on
the device.

  sequential   per window four orbx_lk_track calls (host frames and host points in, host results out; the pyramid of
               the previous `next` frame is reused through prev == NULL), the survivors compacted on the host between
               the calls -- what orbx::track_points_across_window does
  one launch   orbx_lk_track_windows_device on the device-resident frames with the corner block's pointers, then
               orbx_lk_windows_fetch (the results on the host, as above)
  with upload  the same, but the frames start on the host as they do for the sequential path: the upload of every
               frame of the batch is inside the timed region

Each is timed with the host clock around work that ends in a synchronise, after a warm-up, --reps times in turn
(sequential, one launch, with upload, sequential, ...).  The results of the paths are compared bit for bit.  One JSON
line.

The kernels are timed in a SECOND run, under the profiler:
  rocprofv3 --kernel-trace --stats -d out/lk_windows -o lk_windows --output-format csv -- \\
      python tools/lk_window_probe.py --windows 50 --reps 1
and `--stages <kernel_stats.csv>` prints the k_lk_* rows of such a file.

  python tools/lk_window_probe.py [--windows 1 50] [--reps 3]
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW_LEN, SLOTS = 5, 2000
GFTT = (2000, 0.01, 8.0)
LK = dict(win=21, max_level=3, max_iters=30, epsilon=0.01)


def stages(path):
    out = {}
    for r in csv.DictReader(open(path)):
        if "k_lk_" in r["Name"]:
            name = r["Name"][r["Name"].index("k_lk_"):].split("(")[0]
            out[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                         "us_per_call": float(r["AverageNs"]) / 1e3}
    return out


def sequential(c, host_frames, firsts, corners):
    """tracks (windows, SLOTS, WINDOW_LEN, 2) and seen (windows, SLOTS) through four lk_track calls per window"""
    tracks = np.zeros((len(firsts), SLOTS, WINDOW_LEN, 2), np.float32)
    seen = np.zeros((len(firsts), SLOTS), np.int32)
    for w, f0 in enumerate(firsts):
        cur = corners[w]
        live = np.arange(len(cur))
        tracks[w, live, 0] = cur
        seen[w, live] = 1
        for k in range(1, WINDOW_LEN):
            if len(live) == 0:
                break
            out, st, _ = c.lk_track(host_frames[f0] if k == 1 else None, host_frames[f0 + k], cur, **LK)
            ok = st == 1
            live, cur = live[ok], out[ok]
            tracks[w, live, k] = cur
            seen[w, live] = k + 1
    return tracks, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", help="a rocprofv3 kernel_stats.csv of this probe: print the k_lk_* rows and exit")
    a = ap.parse_args()
    if a.stages:
        print(json.dumps(stages(a.stages)))
        return
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    out = {"window_len": WINDOW_LEN, "slots": SLOTS, "reps": a.reps, "runs": []}
    for nw in a.windows:
        nf = nw + WINDOW_LEN - 1
        frames = pkg.streams.stream_a_device(torch, 0, nf, "cuda")
        _, h, w = frames.shape
        host_frames = frames.cpu().numpy()
        firsts = np.arange(nw, dtype=np.int32)
        torch.cuda.synchronize()
        p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=nf, nlevels=1)
        with pkg.Context(p) as c:
            c.good_features_batch(frames[:nw], *GFTT)
            corners = c.good_features_fetch()
            v = c.good_features_view()
            pts = np.zeros((nw, SLOTS, 2), np.float32)
            for i, xy in enumerate(corners):
                pts[i, :len(xy)] = xy
            counts = np.int32([len(xy) for xy in corners])

            def one_launch():
                c.lk_track_windows(frames, firsts, WINDOW_LEN, v.corners_xy, v.counts, slot_capacity=v.slot_capacity,
                                   **LK)
                return c.lk_windows_fetch()

            def with_upload():
                c.lk_track_windows(host_frames, firsts, WINDOW_LEN, pts, counts, **LK)
                return c.lk_windows_fetch()

            paths = [("sequential", lambda: sequential(c, host_frames, firsts, corners)), ("one_launch", one_launch),
                     ("one_launch_with_upload", with_upload)]
            res = {name: f() for name, f in paths}  # warm-up: code objects, workspaces, result blocks
            ms = {name: [] for name, _ in paths}
            for _ in range(a.reps):
                for name, f in paths:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            # the launch alone, on the device clock
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s = torch.cuda.Stream()
            s.synchronize()
            e0.record(s)
            c.lk_track_windows(frames, firsts, WINDOW_LEN, v.corners_xy, v.counts, slot_capacity=v.slot_capacity,
                               stream=s.cuda_stream, **LK)
            e1.record(s)
            e1.synchronize()
            run = {"windows": nw, "frames": nf, "width": w, "height": h, "points_mean": float(counts.mean()),
                   "survive_all_frames": float((res["sequential"][1] == WINDOW_LEN).sum() / max(counts.sum(), 1)),
                   "one_launch_device_ms": e0.elapsed_time(e1)}
            for name, _ in paths:
                run[name + "_ms"] = ms[name]
                run[name + "_ms_median"] = float(np.median(ms[name]))
            same = True
            for name in ("one_launch", "one_launch_with_upload"):
                same &= np.array_equal(res[name][1], res["sequential"][1])
                same &= np.array_equal(res[name][0].view(np.uint32), res["sequential"][0].view(np.uint32))
            run["bit_identical"] = bool(same)
            out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
