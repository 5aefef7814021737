"""Times orbx_batch_scale_consecutive on 1023 pairs of real frames, next to the steps before it.

The batch alternates the two golden KITTI frames (f0, f1, f0, ...), so every pair has real parallax.  In one
process: the detection step (device-resident frames), the match step, orbx_batch_pose_consecutive and
orbx_batch_scale_consecutive, each as a host clock around the launch and a device sync, after warm-up, best and
median of --reps.  Also one single-core run of the sequential restatement (tests/cpp/scale_sequential.cpp) over
the same match lists and poses.

  python tools/scale_probe.py [--frames 1024] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
DP = C.POINTER(C.c_double)


def timed(reps, launch, sync):
    for _ in range(2):  # warm-up
        launch()
        sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        launch()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_best": min(ms), "ms_median": float(np.median(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nfeatures", type=int, default=3000, help="the reference's cv::ORB::create(3000)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the single-core sequential comparison")
    a = ap.parse_args()
    import torch

    import __graft_entry__

    pkg = __graft_entry__.load_package()
    k0, k1 = pkg.streams.load_kitti(0), pkg.streams.load_kitti(1)
    h, w = k0.shape
    frames = np.stack([k0 if i % 2 == 0 else k1 for i in range(a.frames)])
    npairs = a.frames - 1
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", nfeatures=a.nfeatures, max_width=w, max_height=h, max_batch=a.frames)
    with pkg.Context(p) as c:
        cap = c.plan(w, h)["out_capacity"]
        out = {"pairs": npairs, "nfeatures": a.nfeatures}
        out["detect"] = timed(a.reps, lambda: c.batch_device(d.data_ptr(), a.frames, w, h), c.wait)
        out["match"] = timed(a.reps, lambda: c.batch_match_consecutive(0.8), c.wait)
        out["pose"] = timed(a.reps, lambda: c.batch_pose_consecutive(K), lambda: c.batch_pose_fetch(0, 1))
        out["scale"] = timed(a.reps, lambda: c.batch_scale_consecutive(K), lambda: c.batch_scale_fetch(0, 1))
        out["scale"]["us_per_pair"] = out["scale"]["ms_best"] * 1e3 / npairs
        r = c.batch_scale_fetch()
        out.update(scale_pair1_pair2=[float(v) for v in r["scale"][1:3]], triplets_mean=float(r["triplets"][1:].mean()),
                   ratios_mean=float(r["ratios_used"][1:].mean()))
        if not a.no_cpu:
            kps = c.batch_fetch(0, 4, cap)["kps"]
            poses = c.batch_pose_fetch(0, 3)
            lists = []
            for i in range(3):
                qi, ti, _ = c.batch_match_fetch(i, cap)
                lists.append((qi, ti, np.ascontiguousarray(kps[i][qi], np.float32),
                              np.ascontiguousarray(kps[i + 1][ti], np.float32)))
            out["matches_pair0_pair1"] = [len(lists[0][0]), len(lists[1][0])]
    if not a.no_cpu:
        with tempfile.TemporaryDirectory() as td:
            so = os.path.join(td, "seq.so")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                                   "-o", so, os.path.join(ROOT, "tests", "cpp", "scale_sequential.cpp")])
            lib = C.CDLL(so)
            lib.seq_join_scale.restype = C.c_double
            Kc = np.ascontiguousarray(K)
            # the batch holds only two distinct pairs: time each pair's triangulation + join once and scale to the batch
            tri = []
            for i, (qi, ti, p1, p2) in enumerate(lists):
                n = len(p1)
                xyz, valid = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.uint8)
                R, t = np.ascontiguousarray(poses["R"][i]), np.ascontiguousarray(poses["t"][i])
                s0 = time.perf_counter()
                lib.seq_triangulate(C.c_void_p(p1.ctypes.data), C.c_void_p(p2.ctypes.data), n, Kc.ctypes.data_as(DP),
                                    R.ctypes.data_as(DP), t.ctypes.data_as(DP), C.c_void_p(xyz.ctypes.data),
                                    C.c_void_p(valid.ctypes.data))
                tri.append(((time.perf_counter() - s0) * 1e3, xyz, valid, R, t))
            per = []
            for i in (1, 2):
                t0 = np.ascontiguousarray(lists[i - 1][1], np.int32)
                q1 = np.ascontiguousarray(lists[i][0], np.int32)
                nt, used = C.c_int(0), C.c_int(0)
                s0 = time.perf_counter()
                s = lib.seq_join_scale(C.c_void_p(t0.ctypes.data), len(t0),
                                       C.c_void_p(tri[i - 1][1].ctypes.data), C.c_void_p(tri[i - 1][2].ctypes.data),
                                       tri[i - 1][3].ctypes.data_as(DP), tri[i - 1][4].ctypes.data_as(DP),
                                       C.c_void_p(q1.ctypes.data), len(q1), C.c_void_p(tri[i][1].ctypes.data),
                                       C.c_void_p(tri[i][2].ctypes.data), None, None, C.byref(nt), C.byref(used))
                per.append(tri[i][0] + (time.perf_counter() - s0) * 1e3)
                assert s == out["scale_pair1_pair2"][i - 1], (s, out["scale_pair1_pair2"])
            out["cpu_seq_ms_per_pair"] = per
            out["cpu_seq_ms_batch_estimate"] = per[0] * ((npairs + 1) // 2) + per[1] * (npairs // 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
