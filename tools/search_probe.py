"""Measures rank 21: the gated re-association beside the ungated one on the same sets, and
the projection of a landmarks block, all on the device.

  sets      --windows windows of --slots x --slots described slots, every slot ORBX_PD_OK: train descriptors of random
            bytes at positions spread uniformly over --width x --height; query q is a copy of a random train slot with
            0 .. 19 bits flipped, within 5 pixels of it
  ungated   orbx_reassociate_device(query, train), ratio 0.8, max_distance 64, unique 1
  gated     orbx_reassociate_gated_device on the same sets with the positions, --radius pixels, accept_lone 1
  project   orbx_landmarks_project_device on a landmarks block of --windows windows of 200 slots (carry_ref streams)

The two re-associations ALTERNATE in one process, --reps of each after one warm-up pair; a host clock runs around each
call (enqueue, then a device-wide wait): best, median and all of them.  Pairs per query: the candidates (rule L) from
the call's own block, and the pairs LOOKED AT, recounted on the host for the first --sample windows from the grid the
kernel documents (csrc/orbx_search.hip: k_sg_bin).  Kernel times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/search_probe.py --reps 3

  python tools/search_probe.py [--windows 1024] [--slots 2000] [--radius 20] [--reps 10]
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

CELLS_MAX = 4096  # = ORBX_SG_CELLS_MAX


def timed(call, wait):
    wait()
    t0 = time.perf_counter()
    call()
    wait()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return {"best_ms": min(ms), "median_ms": float(np.median(ms)), "all_ms": [round(t, 3) for t in ms]}


def looked_at(qxy, txy, radius):
    """pairs one window's queries look at: k_sg_bin's grid and k_sg_knn2's walk, recounted with numpy"""
    x0, y0 = qxy[:, 0].min() - radius, qxy[:, 1].min() - radius
    ex, ey = qxy[:, 0].max() + radius - x0, qxy[:, 1].max() + radius - y0
    side = max(radius, np.sqrt(ex * ey / (CELLS_MAX // 2)))
    nx = int(min(np.floor(ex / side) + 1, 256))
    ny = int(min(np.floor(ey / side) + 1, CELLS_MAX // nx))
    cell = lambda v, o, n: np.clip(np.floor((v - o) / side), 0, n - 1).astype(np.int64)
    hist = np.zeros((ny, nx), np.int64)
    np.add.at(hist, (cell(txy[:, 1], y0, ny), cell(txy[:, 0], x0, nx)), 1)
    cum = np.zeros((ny + 1, nx + 1), np.int64)
    cum[1:, 1:] = hist.cumsum(0).cumsum(1)
    cx0, cx1 = cell(qxy[:, 0] - radius, x0, nx), cell(qxy[:, 0] + radius, x0, nx) + 1
    cy0, cy1 = cell(qxy[:, 1] - radius, y0, ny), cell(qxy[:, 1] + radius, y0, ny) + 1
    seen = cum[cy1, cx1] - cum[cy0, cx1] - cum[cy1, cx0] + cum[cy0, cx0]
    return float(seen.mean()), nx, ny, float(side)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--width", type=int, default=1241)
    ap.add_argument("--height", type=int, default=376)
    ap.add_argument("--radius", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=8)
    a = ap.parse_args()
    import torch

    import __graft_entry__
    import carry_ref as CR

    pkg = __graft_entry__.load_package()
    RL, SE = pkg.orbx_reloc, pkg.orbx_search
    n, cap = a.windows, a.slots
    gen = torch.Generator(device="cuda").manual_seed(21)
    rnd = lambda *shape: torch.rand(*shape, generator=gen, device="cuda", dtype=torch.float64)
    tdesc = torch.randint(0, 256, (n, cap, 32), generator=gen, device="cuda", dtype=torch.uint8)
    txy = torch.stack([rnd(n, cap) * (a.width - 1), rnd(n, cap) * (a.height - 1)], dim=-1).contiguous()
    src = torch.randint(0, cap, (n, cap), generator=gen, device="cuda")
    qdesc = torch.gather(tdesc, 1, src[..., None].expand(-1, -1, 32)).clone()
    flips = torch.randint(0, 20, (n, cap), generator=gen, device="cuda")
    for k in range(19):  # flip bit k of byte k of every query with more than k flips
        qdesc[:, :, k] ^= ((flips > k).to(torch.uint8) << (k % 8))
    qxy = (torch.gather(txy, 1, src[..., None].expand(-1, -1, 2)) + (rnd(n, cap, 2) * 10 - 5)).to(torch.float32)
    qxy = qxy.contiguous()
    state = torch.full((n, cap), RL.PD_OK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {"windows": n, "slots": cap, "width": a.width, "height": a.height, "radius_px": a.radius, "reps": a.reps}
    wait = torch.cuda.synchronize  # (the whole device: the context's stream is its own)
    common = dict(ratio=0.8, max_distance=64, unique=1)
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160)) as c:
        ungated = lambda: RL.reassociate(c, qdesc, state, tdesc, state, **common)
        gated = lambda: SE.reassociate_gated(c, qdesc, state, qxy, tdesc, state, txy, None, radius_px=a.radius,
                                             accept_lone=1, **common)
        times = {"ungated": [], "gated": []}
        for rep in range(a.reps + 1):  # the first pair grows the buffers
            for name, call in (("ungated", ungated), ("gated", gated)):
                ms = timed(call, wait)
                if rep:
                    times[name].append(ms)
        res["reassociate"], res["reassociate_gated"] = summary(times["ungated"]), summary(times["gated"])
        res["all_gated_below_all_ungated"] = max(times["gated"]) < min(times["ungated"])
        res["ratio_of_medians"] = res["reassociate"]["median_ms"] / res["reassociate_gated"]["median_ms"]
        ungated()
        plain = RL.reassociate_fetch(c)
        gated()
        got, cand = RL.reassociate_fetch(c), SE.reassociate_gated_fetch(c)
        right = src.cpu().numpy()
        res["matches_ungated"] = int(plain["count"].sum())
        res["matches_ungated_right"] = int(((plain["origin"] == right) & (plain["origin"] >= 0)).sum())
        res["matches_gated"] = int(got["count"].sum())
        res["matches_gated_right"] = int(((got["origin"] == right) & (got["origin"] >= 0)).sum())
        res["candidates_per_query"] = float(cand.mean())
        res["pairs_per_query_ungated"] = cap
        hq, ht = qxy[:a.sample].cpu().numpy().astype(np.float64), txy[:a.sample].cpu().numpy()
        seen = [looked_at(hq[w], ht[w], a.radius) for w in range(min(a.sample, n))]
        res["pairs_looked_at_per_query"] = float(np.mean([s[0] for s in seen]))
        res["grid"] = {"nx": seen[0][1], "ny": seen[0][2], "side_px": seen[0][3]}

        # the projection: --windows old windows of 200 slots under their own last pose
        m = min(n, 1024)
        wins = [CR.two_generations(4000 + w % 16, 4, 200, 0, min_seen=2)[1] for w in range(16)]
        tracks = np.stack([wins[w % 16]["tracks"] for w in range(m)])
        seenw = np.stack([wins[w % 16]["seen"] for w in range(m)])
        poses = np.stack([wins[w % 16]["true_poses"] for w in range(m)])
        c.landmarks_build(CR.K, tracks, seenw, poses)
        last = torch.from_numpy(np.ascontiguousarray(poses[:, -1])).cuda()
        torch.cuda.synchronize()
        project = lambda: SE.landmarks_project(c, CR.K, last, a.width, a.height, 8.0)
        ms = [timed(project, wait) for _ in range(a.reps + 1)][1:]
        res["landmarks_project"] = summary(ms)
        res["projected_ok"] = int(SE.landmarks_project_fetch(c)["count"].sum())
        res["projected_windows"], res["projected_slots"] = m, 200
    print(json.dumps(res))


if __name__ == "__main__":
    main()
