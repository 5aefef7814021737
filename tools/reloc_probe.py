"""Measures rank 19: ORB descriptors at caller-held points of many frames per call, and the
re-association of two described sets, all on the device.

  frames    --frames copies of kitti_000000, frame f rolled f % 61 pixels to the left (so that consecutive frames
            differ); the "other view" of frame f is the same image rolled 5 pixels further
  points    orbx_good_features_batch_device on both sets, --slots corners per frame at most
  describe  orbx_describe_points_device from the good-features view: the first set into bank 0, the other into bank 1
  join      orbx_reassociate_device(query = bank 1, train = bank 0): --frames windows at --slots x --slots
  beside    one orbx_detect_and_compute_batch_device of the first set, so that k_describe2 stands in the same trace

A host clock runs around each call (enqueue, then a device-wide wait) after a warm-up: best and median of
--reps.  Kernel times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/reloc_probe.py --reps 3

  python tools/reloc_probe.py [--frames 1024] [--slots 2000] [--reps 10] [--blur-levels 0]
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


def clock(call, wait, reps):
    ms = []
    for _ in range(reps + 1):  # the first repetition grows the buffers
        wait()
        t0 = time.perf_counter()
        call()
        wait()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": min(ms[1:]), "median_ms": float(np.median(ms[1:])), "all_ms": [round(t, 3) for t in ms[1:]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blur-levels", type=int, default=0)
    ap.add_argument("--quality", type=float, default=0.01)
    ap.add_argument("--min-distance", type=float, default=7.0)
    a = ap.parse_args()
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    RL = pkg.orbx_reloc
    n = a.frames
    base = torch.from_numpy(pkg.streams.load_kitti(0)).cuda()
    h, w = base.shape
    first = torch.stack([torch.roll(base, -(f % 61), 1) for f in range(n)])
    other = torch.stack([torch.roll(base, -(f % 61) - 5, 1) for f in range(n)])
    torch.cuda.synchronize()
    res = {"frames": n, "slots": a.slots, "width": w, "height": h, "blur_levels": a.blur_levels, "reps": a.reps}
    params = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=n, blur_levels=a.blur_levels)
    with pkg.Context(params) as c:
        # the points: the corners of both sets, kept in tensors of the probe's own (the view is replaced by the next call)
        pts, cnt = [], []
        for frames in (first, other):
            c.good_features_batch(frames, a.slots, a.quality, a.min_distance)
            got = c.good_features_fetch()
            cap = c.good_features_view().slot_capacity
            counts = np.array([len(g) for g in got], np.int32)
            corners = np.zeros((n, cap, 2), np.float32)
            for f, g in enumerate(got):
                corners[f, :len(g)] = g
            pts.append(torch.from_numpy(corners).cuda())
            cnt.append(torch.from_numpy(counts).cuda())
        torch.cuda.synchronize()
        cap = pts[0].shape[1]
        res["slot_capacity"] = cap
        res["corners_per_frame_median"] = [float(np.median(x.cpu().numpy())) for x in cnt]

        wait = torch.cuda.synchronize  # (the whole device: the context's stream is its own)

        def describe(bank):
            RL.describe_points(c, (first, other)[bank], pts[bank], bank=bank, counts=cnt[bank])

        res["describe_bank0"] = clock(lambda: describe(0), wait, a.reps)
        res["describe_bank1"] = clock(lambda: describe(1), wait, a.reps)
        d0, d1 = RL.point_descriptors_fetch(c, 0), RL.point_descriptors_fetch(c, 1)
        res["described_points"] = [int(d0["n_ok"].sum()), int(d1["n_ok"].sum())]
        res["live_slots"] = [int(cnt[0].sum()), int(cnt[1].sum())]
        q, t = RL.point_descriptors_view(c, 1), RL.point_descriptors_view(c, 0)

        for unique in (1, 0):
            def join():
                RL.reassociate(c, q, train_desc=t, ratio=0.8, max_distance=256, unique=unique)

            res["reassociate_unique_%d" % unique] = clock(join, wait, a.reps)
            got = RL.reassociate_fetch(c)
            res["matches_unique_%d" % unique] = int(got["count"].sum())
            if unique:
                # a match is right when the two corners differ by the 5-pixel roll (no wrap inside the frame)
                o = got["origin"]
                p0, p1 = pts[0].cpu().numpy(), pts[1].cpu().numpy()
                ok = o >= 0
                tr = np.take_along_axis(p0, np.maximum(o, 0)[..., None], axis=1)
                right = ok & (tr[..., 0] - p1[..., 0] == 5.0) & (tr[..., 1] == p1[..., 1])
                res["matches_right"], res["matches_wrong"] = int(right.sum()), int((ok & ~right).sum())
        # the ORB path on the first set, for k_describe2 in the same trace
        c.batch_device(first.data_ptr(), n, w, h)
        c.batch_prefetch(compact=True)
        c.wait()
        res["orb_keypoints"] = int(c.batch_host_view()["counts"].sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
