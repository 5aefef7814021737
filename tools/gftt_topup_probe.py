"""Times orbx_good_features_topup_device against the plain orbx_good_features_batch_device on the same frames.

64 KITTI-shaped frames (stream A of streams.py, device-resident) at (2000, 0.01, 8).  The seeds of a frame are about
two thirds of its own corners (every third one dropped), each moved by a uniform offset within 0.49 px, so the top-up
has to carry ~two thirds of a full frame and find the rest again around them.  Both calls are timed with HIP events
around the enqueue after a warm-up of each, ALTERNATING the two --reps times in one process: best and median of each.

The kernels are timed in a SECOND run, under the profiler (they carry stable names):
  rocprofv3 --kernel-trace --stats -d out/gftt_topup -o gftt_topup --output-format csv -- \
      python tools/gftt_topup_probe.py --reps 3
and `--stages out/gftt_topup/.../gftt_topup_kernel_stats.csv` prints the per-call time of each k_gftt_* kernel.

  python tools/gftt_topup_probe.py [--frames 64] [--reps 10]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAMS = (2000, 0.01, 8.0)


def stages(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_gftt_" in r["Name"]]
    out = {}
    for r in rows:
        name = r["Name"][r["Name"].index("k_gftt_"):].split("(")[0]
        out[name] = {"calls": int(r["Calls"]), "ms_per_call": float(r["AverageNs"]) / 1e6,
                     "total_ms": float(r["TotalDurationNs"]) / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stages", help="a rocprofv3 kernel_stats.csv of this probe: print the k_gftt_* rows and exit")
    a = ap.parse_args()
    if a.stages:
        print(json.dumps(stages(a.stages)))
        return
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    frames = pkg.streams.stream_a_device(torch, 0, a.frames, "cuda")
    n, h, w = frames.shape
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=a.frames, nlevels=1)
    out = {"frames": n, "width": w, "height": h, "params": PARAMS}
    with pkg.Context(p) as c:
        c.good_features_batch(frames, *PARAMS)
        corners = c.good_features_fetch()
        rng = np.random.default_rng(0)
        seeds = np.full((n, PARAMS[0], 2), np.nan, np.float32)
        for f, xy in enumerate(corners):
            keep = xy[np.arange(len(xy)) % 3 != 2]
            seeds[f, :len(keep)] = keep + rng.uniform(-0.49, 0.49, keep.shape)
        d_seeds = torch.from_numpy(seeds).cuda()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()

        def plain():
            c.good_features_batch(frames, *PARAMS, stream=stream.cuda_stream)

        def topup():
            c.good_features_topup(frames, d_seeds, max_corners=PARAMS[0], quality_level=PARAMS[1],
                                  min_distance=PARAMS[2], stream=stream.cuda_stream)

        for _ in range(3):  # warm-up: code objects, the workspace, the bit maps, both result blocks
            plain()
            topup()
        stream.synchronize()
        ms = {"plain": [], "topup": []}
        for _ in range(a.reps):
            for name, call in (("plain", plain), ("topup", topup)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        counts, carried, _, _ = c.good_features_topup_fetch()
        plain_counts = np.array([len(x) for x in corners])
        for name in ms:
            out["%s_ms_best" % name] = min(ms[name])
            out["%s_ms_median" % name] = float(np.median(ms[name]))
            out["%s_ms_all" % name] = [round(v, 4) for v in ms[name]]
        out.update(topup_over_plain_best=min(ms["topup"]) / min(ms["plain"]),
                   topup_over_plain_median=float(np.median(ms["topup"]) / np.median(ms["plain"])),
                   plain_corners_mean=float(plain_counts.mean()), carried_mean=float(carried.mean()),
                   topup_points_mean=float(counts.mean()), new_corners_mean=float((counts - carried).mean()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
