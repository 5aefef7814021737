"""Times orbx_bundle_adjust_batch on 1024 windows of 5 poses x 2000 landmarks.

The windows are the synthetic ones of tests/test_ba.py (sigma = 0.3 px, 10 % outliers, tracks of 2-5 frames);
--distinct of them are generated and repeated to fill the batch.  Timed: a host clock around the entry (host CSR
placement, H2D, the one kernel launch, D2H, sync), after warm-up, best and median of --reps, every call from the same
start.  Also prints the iteration counts and, for scale, one single-core run of the sequential restatement
(tests/cpp/ba_sequential.cpp) over the distinct windows.

  python tools/ba_probe.py [--windows 1024] [--landmarks 2000] [--reps 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--landmarks", type=int, default=2000)
    ap.add_argument("--poses", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="skip the single-core sequential comparison")
    a = ap.parse_args()
    import __graft_entry__
    import test_ba as T

    pkg = __graft_entry__.load_package()
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    wins = [T.make_window(900 + i, a.poses, a.landmarks, sigma=0.3, outliers=0.1) for i in range(min(a.distinct, a.windows))]
    pick = [wins[i % len(wins)] for i in range(a.windows)]
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([w[k] for w in pick]), dt)
    off = lambda k: np.concatenate([[0], np.cumsum([len(w[k]) for w in pick])]).astype(np.int32)
    poses0, pts0, xy = cat("poses0", np.float64), cat("pts0", np.float64), cat("obs_xy", np.float64)
    op, oq = cat("obs_point", np.int32), cat("obs_pose", np.int32)
    po, xo, oo = off("poses0"), off("pts0"), off("obs_point")
    K = np.ascontiguousarray(T.K_KITTI)
    out = (pkg.orbx.BaSummary * a.windows)()
    with pkg.Context(pkg.default_params("gpu")) as c:
        f = c._lib.orbx_bundle_adjust_batch

        def once():
            poses, pts = poses0.copy(), pts0.copy()
            t0 = time.perf_counter()
            st = f(c._h, K.ctypes.data_as(DP), a.windows, po.ctypes.data_as(IP), poses.ctypes.data_as(DP),
                   xo.ctypes.data_as(IP), pts.ctypes.data_as(DP), oo.ctypes.data_as(IP), op.ctypes.data_as(IP),
                   oq.ctypes.data_as(IP), xy.ctypes.data_as(DP), 1.0, 200, out)
            ms = (time.perf_counter() - t0) * 1e3
            c._chk(st)
            return ms

        for _ in range(2):  # warm-up: the buffers grow on the first call
            once()
        ms = [once() for _ in range(a.reps)]
    its = np.array([s.iterations for s in out])
    term = np.array([s.termination for s in out])
    res = {"windows": a.windows, "poses": a.poses, "landmarks": a.landmarks, "observations": int(oo[-1]),
           "ms_best": min(ms), "ms_median": float(np.median(ms)), "ms_per_window": min(ms) / a.windows,
           "iters_mean": float(its.mean()), "iters_max": int(its.max()),
           "terminations": [int((term == k).sum()) for k in range(3)]}
    if not a.no_cpu:
        with tempfile.TemporaryDirectory() as td:
            so = os.path.join(td, "seq.so")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                                   "-o", so, os.path.join(ROOT, "tests", "cpp", "ba_sequential.cpp")])
            lib = C.CDLL(so)
            per = []
            for w in wins:
                t0 = time.perf_counter()
                T.seq_ba(lib, w)
                per.append((time.perf_counter() - t0) * 1e3)
        res["cpu_seq_ms_per_window"] = per
        res["cpu_seq_ms_batch_estimate"] = float(np.mean(per)) * a.windows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
