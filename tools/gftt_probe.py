"""Times orbx_good_features_batch_device on 256 KITTI-shaped frames at the reference's (2000, 0.01, 8).

The frames are stream A (streams.py), device-resident.  The call is timed with HIP events around the enqueue, after
warm-up: best and median of --reps.  Next to it one single-core run of the numpy restatement (tests/gftt_ref.py) on
one frame, and a check that frame 0 of the batch equals it.

The three stages are timed in a SECOND run, under the profiler (the kernels carry stable names):
  rocprofv3 --kernel-trace --stats -d out/gftt -o gftt --output-format csv -- \
      python tools/gftt_probe.py --reps 3 --no-cpu
and `--stages out/gftt/.../gftt_kernel_stats.csv` prints the share of each k_gftt_* kernel from such a file.

  python tools/gftt_probe.py [--frames 256] [--reps 10] [--no-cpu]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARAMS = (2000, 0.01, 8.0)


def stages(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_gftt_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for r in rows:
        name = r["Name"][r["Name"].index("k_gftt_"):].split("(")[0]
        out[name] = {"calls": int(r["Calls"]), "ms_per_call": float(r["AverageNs"]) / 1e6,
                     "share": float(r["TotalDurationNs"]) / total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="skip the single-core numpy restatement")
    ap.add_argument("--stages", help="a rocprofv3 kernel_stats.csv of this probe: print the k_gftt_* shares and exit")
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
        stream = torch.cuda.Stream()
        for _ in range(3):  # warm-up: code objects, the workspace, the result block
            c.good_features_batch(frames, *PARAMS, stream=stream.cuda_stream)
        stream.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            c.good_features_batch(frames, *PARAMS, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        got = c.good_features_fetch()
        counts = np.array([len(g) for g in got])
        out.update(ms_best=min(ms), ms_median=float(np.median(ms)), us_per_frame_best=min(ms) * 1e3 / n,
                   corners_mean=float(counts.mean()), corners_min=int(counts.min()), corners_max=int(counts.max()))
        first = frames[0].cpu().numpy()
    if not a.no_cpu:
        import gftt_ref

        gftt_ref.good_features_to_track(first, *PARAMS)  # warm-up
        t0 = time.perf_counter()
        ref, full = gftt_ref.good_features_to_track(first, *PARAMS, full=True)
        out["numpy_one_frame_ms"] = (time.perf_counter() - t0) * 1e3
        out["candidates_frame0"] = len(full["indices"])
        out["frame0_bit_identical"] = bool(ref.shape == got[0].shape and
                                           np.array_equal(ref.view(np.uint32), got[0].view(np.uint32)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
