"""Times tracks -> gated camera -> world poses on windows of 5 frames x 2000 slots, two routes in the same process,
alternating.  Both start from tracks and `seen` on the device and run the tracks pose, the
landmarks build and the solve there; they differ in the two links between them:

  host    the route before rank 14, from entries that route had: orbx_tracks_pose_fetch of R, t and scale, the chain
          on the CPU (orbx_chain_trajectory per window, the closed-form inverse and the quaternion log map in
          vectorised numpy), orbx_landmarks_build_device with those poses from the host, the solve,
          orbx_bundle_adjust_landmarks_fetch of all poses and summaries, the write-back gate in vectorised numpy.
  device  orbx_window_poses_device, orbx_landmarks_build_chained_device, the solve,
          orbx_bundle_adjust_write_back_device, and ONE orbx_bundle_adjust_write_back_fetch at the end.

Both end with the gated 4x4 poses and the updated flags on the host; a host clock runs around each.  The scenes are
those of tests/landmarks_ref.py (sigma = 0.3 px, 10 % outliers on the later frames, tracks of 2-5 frames); --distinct
of them are generated and repeated to fill the batch.  The routes' flags and poses are compared.  After a warm-up of
each route: best and median of --reps.

  python tools/window_poses_probe.py [--windows 64] [--slots 2000] [--reps 10] [--route both|host|device]
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


def blocks_of(C):
    """camera -> world (m, 4, 4) -> world -> camera blocks (m, 6): closed-form inverse, log map through the quaternion"""
    R = np.swapaxes(C[:, :3, :3], 1, 2)
    t = -np.einsum("mij,mj->mi", R, C[:, :3, 3])
    q = np.stack([1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0],
                  R[:, 1, 0] - R[:, 0, 1]], axis=1)
    q /= np.linalg.norm(q, axis=1)[:, None]
    s = np.linalg.norm(q[:, 1:], axis=1)
    f = np.where(s > 0, 2.0 * np.arctan2(s, q[:, 0]) / np.where(s > 0, s, 1.0), 0.0)
    return np.concatenate([q[:, 1:] * f[:, None], t], axis=1)


def rotations_of(w):
    """angle-axis (m, 3) -> rotation matrices (m, 3, 3)"""
    th = np.linalg.norm(w, axis=1)
    k = w / np.where(th > 1e-12, th, 1.0)[:, None]
    Kx = np.zeros((len(w), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * Kx + (1.0 - np.cos(th))[:, None, None] * (Kx @ Kx)


def gate_of(solved, built, converged, max_rot, max_trans):
    """the write-back gate on (m, 6) blocks: gated camera -> world poses (m, 4, 4) and updated (m,)"""
    Rn, Ro = rotations_of(solved[:, :3]), rotations_of(built[:, :3])
    Rd = Rn @ np.swapaxes(Ro, 1, 2)
    cos = np.clip((np.trace(Rd, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    upd = converged & (np.arccos(cos) < max_rot) & (np.linalg.norm(solved[:, 3:] - built[:, 3:], axis=1) < max_trans)
    R = np.where(upd[:, None, None], Rn, Ro)
    t = np.where(upd[:, None], solved[:, 3:], built[:, 3:])
    out = np.zeros((len(solved), 4, 4))
    out[:, :3, :3] = np.swapaxes(R, 1, 2)
    out[:, :3, 3] = -np.einsum("mji,mj->mi", R, t)
    out[:, 3, 3] = 1.0
    return out, upd.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route", choices=("both", "host", "device"), default="both")
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import landmarks_ref as R

    pkg = __graft_entry__.load_package()
    VO = pkg.orbx_vo
    K = np.ascontiguousarray(R.K_KITTI)
    L, n = a.frames, a.windows
    scenes = [R.make_scene(900 + i, W=L, slots=a.slots, sigma=0.3, outliers=0.1, min_seen=2)
              for i in range(min(a.distinct, n))]
    _, tracks, seen = R.stack([scenes[i % len(scenes)] for i in range(n)])
    with pkg.Context(pkg.default_params("gpu")) as c:
        d_tracks, d_seen = torch.from_numpy(tracks).cuda(), torch.from_numpy(seen).cuda()
        torch.cuda.synchronize()
        split = {}

        def host_route():
            t0 = time.perf_counter()
            c.tracks_pose(K, d_tracks, d_seen)
            f = c.tracks_pose_fetch()
            t1 = time.perf_counter()
            Rm, tm, sc = f["R"].reshape(n, L - 1, 3, 3), f["t"].reshape(n, L - 1, 3), f["scale"].reshape(n, L - 1)
            C = np.stack([pkg.chain_trajectory(np.eye(4), Rm[w], tm[w], sc[w]) for w in range(n)])
            poses6 = blocks_of(C.reshape(-1, 4, 4)).reshape(n, L, 6)
            t2 = time.perf_counter()
            c.landmarks_build(K, d_tracks, d_seen, poses6)
            c.bundle_adjust_landmarks()
            solved, sums, _ = c.bundle_adjust_landmarks_fetch(points=False)
            t3 = time.perf_counter()
            conv = np.repeat(np.array([s["termination"] for s in sums]) == pkg.orbx.BA_CONVERGENCE, L)
            p4, upd = gate_of(solved.reshape(-1, 6), poses6.reshape(-1, 6), conv, VO.MAX_ROT_DIFF, VO.MAX_TRANS_DIFF)
            t4 = time.perf_counter()
            split["host"] = {"tracks_pose_and_fetch": t1 - t0, "chain_on_cpu": t2 - t1, "build_solve_fetch": t3 - t2,
                             "gate_on_cpu": t4 - t3}
            return (t4 - t0) * 1e3, p4.reshape(n, L, 4, 4), upd.reshape(n, L)

        def device_route():
            t0 = time.perf_counter()
            c.tracks_pose(K, d_tracks, d_seen)
            VO.window_poses(c)
            VO.landmarks_build_chained(c, K, d_tracks, d_seen)
            c.bundle_adjust_landmarks()
            VO.bundle_adjust_write_back(c)
            t1 = time.perf_counter()
            p4, upd = VO.bundle_adjust_write_back_fetch(c)
            t2 = time.perf_counter()
            split["device"] = {"enqueue": t1 - t0, "wait_and_fetch": t2 - t1}
            return (t2 - t0) * 1e3, p4, upd

        routes = {"host": host_route, "device": device_route}
        names = [a.route] if a.route != "both" else ["host", "device"]
        for name in names:  # warm-up: the buffers grow on the first call
            routes[name]()
        ms = {name: [] for name in names}
        last = {}
        for _ in range(a.reps):
            for name in names:
                t, p4, upd = routes[name]()
                ms[name].append(t)
                last[name] = (p4, upd, dict(split[name]))
        res = {"windows": n, "frames": L, "slots": a.slots, "reps": a.reps}
        for name in names:
            p4, upd, sp = last[name]
            res[name] = {"ms_best": min(ms[name]), "ms_median": float(np.median(ms[name])),
                         "ms_all": [round(x, 2) for x in ms[name]], "updated": int(upd.sum()),
                         "last_split_ms": {k: round(v * 1e3, 3) for k, v in sp.items()}}
        if len(names) == 2:
            res["updated_equal"] = bool(np.array_equal(last["host"][1], last["device"][1]))
            res["poses_max_abs_diff"] = float(np.max(np.abs(last["host"][0] - last["device"][0])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
