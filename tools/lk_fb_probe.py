"""Times the forward-backward check of the windows tracker at the shape of
tools/lk_window_probe.py: stream A (streams.py), 1241 x 376, device-resident; window w covers frames w .. w + 4;
2000 point slots per window, filled by good_features_batch(2000, 0.01, 8) on each window's first frame and left on the
device; LK at (21, 3, 30, 0.01), threshold 1.0.

  plain        orbx_lk_track_windows_device with the corner block's pointers, then orbx_lk_windows_fetch: the tracker
               without the check, the yardstick
  fb           orbx_lk_track_windows_fb_device on the same inputs, then orbx_lk_windows_fetch and
               orbx_lk_windows_fb_fetch
  fb_host      the check on the host: per pair one orbx_lk_track call forward on the live points and one back on the
               survivors (prev == NULL: the pyramid of the forward call's `next` frame is reused), the distance rule
               and the compaction on the host -- what orbx::track_points_across_window_fb does

Each is timed with the host clock around work that ends with the results on the host, after one warm-up, --reps times
in turn (plain, fb, fb_host, plain, ...); the two launches are also timed alone with events on a stream of the
caller's.  fb and fb_host are compared bit for bit, and fb has to be a prefix of plain in every slot.  One JSON line.

The kernels are timed in a SECOND run, under the profiler:
  rocprofv3 --kernel-trace --stats -d out/lk_fb -o lk_fb --output-format csv -- \\
      python tools/lk_fb_probe.py --windows 50 --reps 1
and `--stages <kernel_stats.csv>` prints the k_lk_* rows of such a file.

  python tools/lk_fb_probe.py [--windows 1 50] [--reps 3] [--threshold 1.0] [--max-iters 30]
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


def fb_host(c, host_frames, firsts, corners, thr):
    """tracks, seen and lost through two lk_track calls per pair, rule 3 and the compaction on the host"""
    tracks = np.zeros((len(firsts), SLOTS, WINDOW_LEN, 2), np.float32)
    seen = np.zeros((len(firsts), SLOTS), np.int32)
    lost = np.zeros((len(firsts), SLOTS), np.int32)
    thr2 = np.float64(np.float32(thr)) ** 2
    for w, f0 in enumerate(firsts):
        cur = corners[w]
        live = np.arange(len(cur))
        tracks[w, live, 0] = cur
        seen[w, live] = 1
        for k in range(1, WINDOW_LEN):
            if len(live) == 0:
                break
            q, st, _ = c.lk_track(host_frames[f0 + k - 1], host_frames[f0 + k], cur, **LK)
            ok = st == 1
            lost[w, live[~ok]] = 1
            live, cur, q = live[ok], cur[ok], q[ok]
            if len(live) == 0:
                break
            r, st, _ = c.lk_track(None, host_frames[f0 + k - 1], q, **LK)
            ok = st == 1
            lost[w, live[~ok]] = 2
            live, cur, q, r = live[ok], cur[ok], q[ok], r[ok]
            d = (r - cur).astype(np.float64)
            ok = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= thr2
            lost[w, live[~ok]] = 3
            live, cur = live[ok], q[ok]
            tracks[w, live, k] = cur
            seen[w, live] = k + 1
    return tracks, seen, lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--max-iters", type=int, default=LK["max_iters"],
                    help="0: no Newton steps, i.e. what a pass costs besides them (templates, the error pass)")
    ap.add_argument("--stages", help="a rocprofv3 kernel_stats.csv of this probe: print the k_lk_* rows and exit")
    a = ap.parse_args()
    if a.stages:
        print(json.dumps(stages(a.stages)))
        return
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    thr = a.threshold
    LK["max_iters"] = a.max_iters
    out = {"window_len": WINDOW_LEN, "slots": SLOTS, "reps": a.reps, "threshold": thr, "lk": LK, "runs": []}
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
            counts = np.int32([len(xy) for xy in corners])
            args = (frames, firsts, WINDOW_LEN, v.corners_xy, v.counts)

            def plain():
                c.lk_track_windows(*args, slot_capacity=v.slot_capacity, **LK)
                return c.lk_windows_fetch()

            def fb():
                c.lk_track_windows(*args, slot_capacity=v.slot_capacity, fb_threshold=thr, **LK)
                return c.lk_windows_fetch() + c.lk_windows_fb_fetch()

            paths = [("plain", plain), ("fb", fb), ("fb_host", lambda: fb_host(c, host_frames, firsts, corners, thr))]
            res = {name: f() for name, f in paths}  # warm-up: code objects, workspaces, result blocks
            ms = {name: [] for name, _ in paths}
            for _ in range(a.reps):
                for name, f in paths:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            # the launches alone, on the device clock, in turn
            s = torch.cuda.Stream()
            dev = {"plain": [], "fb": []}
            for _ in range(a.reps):
                for name, kw in (("plain", {}), ("fb", {"fb_threshold": thr})):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.synchronize()
                    e0.record(s)
                    c.lk_track_windows(*args, slot_capacity=v.slot_capacity, stream=s.cuda_stream, **kw, **LK)
                    e1.record(s)
                    e1.synchronize()
                    dev[name].append(e0.elapsed_time(e1))
            tracks, seen, err, d2, lost = res["fb"]
            used = np.arange(SLOTS)[None] < counts[:, None]
            run = {"windows": nw, "frames": nf, "width": w, "height": h, "points_mean": float(counts.mean()),
                   "plain_survive_all_frames": float((res["plain"][1] == WINDOW_LEN).sum() / max(counts.sum(), 1)),
                   "lost_share": {name: float(((lost == k) & used).sum() / max(counts.sum(), 1))
                                  for k, name in enumerate(("alive", "forward", "backward", "distance"))},
                   "fb_d2_median_of_passed": float(np.median(d2[np.arange(1, WINDOW_LEN)[None, None] < seen[..., None]])),
                   "device_ms": dev}
            for name, _ in paths:
                run[name + "_ms"] = ms[name]
                run[name + "_ms_median"] = float(np.median(ms[name]))
                run[name + "_ms_spread"] = float(max(ms[name]) - min(ms[name]))
            run["fb_over_plain"] = run["fb_ms_median"] / run["plain_ms_median"]
            run["fb_host_over_fb"] = run["fb_host_ms_median"] / run["fb_ms_median"]
            run["fb_over_plain_device"] = float(np.median(dev["fb"]) / np.median(dev["plain"]))
            ht, hs, hl = res["fb_host"]
            run["fb_equals_fb_host"] = bool(np.array_equal(seen, hs) and np.array_equal(lost, hl) and
                                            np.array_equal(tracks.view(np.uint32), ht.view(np.uint32)))
            pt, ps, _ = res["plain"]
            m = np.arange(WINDOW_LEN)[None, None] < seen[..., None]
            run["fb_is_prefix_of_plain"] = bool((seen <= ps).all() and
                                                np.array_equal(tracks.view(np.uint32)[m], pt.view(np.uint32)[m]))
            out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
