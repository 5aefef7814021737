"""Times orbx_batch_pose_consecutive on 1023 pairs of real frames.

The batch alternates the two golden KITTI frames (f0, f1, f0, ...), so every pair has real parallax.
Kernel time: a host clock around the launch and a device sync, after warm-up, best and median of
--reps.  Also prints iterations per pair and, for comparison, one single-core run of the sequential
restatement (tests/cpp/pose_sequential.cpp) over the same point lists.

  python tools/pose_probe.py [--frames 1024] [--reps 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nfeatures", type=int, default=3000, help="the reference's cv::ORB::create(3000)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the single-core sequential comparison")
    a = ap.parse_args()
    import __graft_entry__

    pkg = __graft_entry__.load_package()
    k0, k1 = pkg.streams.load_kitti(0), pkg.streams.load_kitti(1)
    h, w = k0.shape
    frames = np.stack([k0 if i % 2 == 0 else k1 for i in range(a.frames)])
    npairs = a.frames - 1
    p = pkg.default_params("gpu", nfeatures=a.nfeatures, max_width=w, max_height=h, max_batch=a.frames)
    with pkg.Context(p) as c:
        cap = c.plan(w, h)["out_capacity"]
        c.batch_host(frames)
        c.batch_match_consecutive(0.8)
        for _ in range(2):  # warm-up
            c.batch_pose_consecutive(K)
            c.batch_pose_fetch(0, 1)
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            c.batch_pose_consecutive(K)
            c.batch_pose_fetch(0, 1)  # synchronises the batch's stream
            ms.append((time.perf_counter() - t0) * 1e3)
        r = c.batch_pose_fetch()
        nmatch = [len(c.batch_match_fetch(i, cap)[0]) for i in (0, 1)]
        out = {"pairs": npairs, "ms_best": min(ms), "ms_median": float(np.median(ms)),
               "us_per_pair": min(ms) * 1e3 / npairs, "iters_mean": float(r["iters"].mean()),
               "iters_max": int(r["iters"].max()), "inliers_mean": float(r["inliers"].mean()),
               "matches_pair0_pair1": nmatch, "nfeatures": a.nfeatures}
        if not a.no_cpu:
            kps = c.batch_fetch(0, 3, cap)["kps"]
            pts = []
            for i in (0, 1):
                qi, ti, _ = c.batch_match_fetch(i, cap)
                pts.append((np.ascontiguousarray(kps[i][qi], np.float32), np.ascontiguousarray(kps[i + 1][ti], np.float32)))
    if not a.no_cpu:
        with tempfile.TemporaryDirectory() as td:
            so = os.path.join(td, "seq.so")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                                   "-o", so, os.path.join(ROOT, "tests", "cpp", "pose_sequential.cpp")])
            lib = C.CDLL(so)
            Kc = np.ascontiguousarray(K)
            # the batch holds only two distinct pairs: time each once and scale to the batch
            per = []
            for p1, p2 in pts:
                n = len(p1)
                E, R, t = np.zeros(9), np.zeros(9), np.zeros(3)
                mask = np.zeros(max(n, 1), np.uint8)
                ii = [C.c_int(0) for _ in range(3)]
                s0 = time.perf_counter()
                lib.seq_estimate_pose(C.c_void_p(p1.ctypes.data), C.c_void_p(p2.ctypes.data), n,
                                      Kc.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(0.999), C.c_double(1.0), 1000,
                                      C.c_uint64(0), C.c_void_p(E.ctypes.data), C.c_void_p(R.ctypes.data),
                                      C.c_void_p(t.ctypes.data), C.c_void_p(mask.ctypes.data), C.byref(ii[0]),
                                      C.byref(ii[1]), C.byref(ii[2]))
                per.append((time.perf_counter() - s0) * 1e3)
            out["cpu_seq_ms_per_pair"] = per
            out["cpu_seq_ms_batch_estimate"] = (per[0] * ((npairs + 1) // 2) + per[1] * (npairs // 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
