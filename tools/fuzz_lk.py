"""Random-configuration parity hunt for the LK tracker: HIP path vs oracle/lk_oracle.c, bit for bit.
usage: python tools/fuzz_lk.py [seconds] [seed] [only_iteration]   (the third argument replays one iteration verbosely)
       python tools/fuzz_lk.py --windows [seconds] [seed]
--windows: random batches of windows through orbx_lk_track_windows_device (random window starts and lengths, ragged
counts, strided frames, a random workspace limit) against the oracle chain of tests/lk_window_ref.py."""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("visual-odometry-gpu_amd")
import oracle_lib as O

windows_mode = "--windows" in sys.argv
sys.argv = [a for a in sys.argv if a != "--windows"]
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
only = int(sys.argv[3]) if len(sys.argv) > 3 else -1
k0 = O.load_kitti(0)


def fuzz_windows():
    import torch
    import lk_window_ref as R

    t0 = time.time(); it = 0; nslots = 0
    with pkg.Context(pkg.default_params("gpu", max_width=200, max_height=160, max_batch=12, nlevels=1)) as c:
        while time.time() - t0 < budget:
            h, w, nf = int(rng.integers(8, 161)), int(rng.integers(8, 201)), int(rng.integers(2, 13))
            y0, x0 = int(rng.integers(0, 376 - h - 40)), int(rng.integers(0, 1241 - w - 40))
            frames = np.stack([k0[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w] for dy, dx in
                               np.cumsum(rng.integers(0, 4, (nf, 2)), 0)])
            if rng.random() < 0.3:
                frames = np.clip(frames.astype(np.int16) + rng.integers(-6, 7, frames.shape), 0, 255).astype(np.uint8)
            wl, nw, cap = int(rng.integers(2, nf + 1)), int(rng.integers(1, 7)), int(rng.integers(1, 200))
            first = rng.integers(0, nf - wl + 1, nw).astype(np.int32)
            pts = np.stack([rng.uniform(-40, w + 40, (nw, cap)), rng.uniform(-40, h + 40, (nw, cap))], 2).astype(np.float32)
            counts = rng.integers(0, cap + 3, nw).astype(np.int32) if rng.random() < 0.7 else None
            kw = dict(win=int(rng.choice([21, 21, int(rng.integers(3, 32))])), max_level=int(rng.integers(0, 8)),
                      max_iters=int(rng.integers(0, 40)), epsilon=float(rng.choice([0.0, 0.001, 0.01, 0.03, 0.5])))
            rs_ = w + int(rng.integers(0, 20))
            fs_ = rs_ * h + int(rng.integers(0, 50))
            buf = rng.integers(0, 256, 5 + nf * fs_, dtype=np.uint8)
            np.lib.stride_tricks.as_strided(buf[5:], shape=(nf, h, w), strides=(fs_, rs_, 1))[...] = frames
            t = torch.as_strided(torch.from_numpy(buf).cuda(), (nf, h, w), (fs_, rs_, 1), 5)
            c.lk_workspace_limit(int(rng.choice([0, 1, 6 * h * w * int(rng.integers(2, 13))])))
            c.lk_track_windows(t, first, wl, pts, counts, **kw)
            got = c.lk_windows_fetch()
            ref = R.track_windows(frames, first, wl, pts, counts, **kw)
            ok = np.array_equal(got[1], ref[1]) and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and \
                np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
            assert ok, (it, h, w, nf, wl, list(first), cap, counts, kw)
            it += 1; nslots += nw * cap
    print("lk windows fuzz ok: %d batches, %d slots in %.0f s" % (it, nslots, time.time() - t0))


if windows_mode:
    fuzz_windows()
    sys.exit(0)
p = pkg.default_params("gpu", max_width=64, max_height=64, max_batch=1, nlevels=1)
t0 = time.time(); it = 0; npts = 0
with pkg.Context(p) as c:
    while time.time() - t0 < budget:
        h, w = int(rng.integers(8, 300)), int(rng.integers(8, 400))
        kind = rng.integers(0, 4)
        if kind == 0:
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == 1:
            y0, x0 = int(rng.integers(0, 376 - h)), int(rng.integers(0, 1241 - w))
            a = np.ascontiguousarray(k0[y0:y0 + h, x0:x0 + w])
        elif kind == 2:
            a = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
            a[rng.integers(0, h, 20), rng.integers(0, w, 20)] = 255
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            a = ((np.sin(xx * 0.2) * np.cos(yy * 0.13) + 1) * 127).astype(np.uint8)
        b = np.roll(a, (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))), (0, 1))
        if rng.random() < 0.3:
            b = np.clip(b.astype(np.int16) + rng.integers(-6, 7, b.shape), 0, 255).astype(np.uint8)
        n = int(rng.integers(0, 300))
        pts = np.stack([rng.uniform(-40, w + 40, n), rng.uniform(-40, h + 40, n)], 1).astype(np.float32)
        kw = dict(win=int(rng.integers(3, 32)), max_level=int(rng.integers(0, 8)), max_iters=int(rng.integers(0, 40)),
                  epsilon=float(rng.choice([0.0, 0.001, 0.01, 0.03, 0.5])))
        if only >= 0 and it != only:
            it += 1
            if it > only:
                break
            continue
        ro, rs, re, _ = O.lk_track(a, b, pts, **kw)
        go, gs, ge = c.lk_track(a, b, pts, **kw)
        ok = np.array_equal(gs, rs) and np.array_equal(go.view(np.uint32), ro.view(np.uint32)) and \
            np.array_equal(ge.view(np.uint32), re.view(np.uint32))
        if not ok:
            bad = np.nonzero((gs != rs) | (go.view(np.uint32) != ro.view(np.uint32)).any(1) | (ge.view(np.uint32) != re.view(np.uint32)))[0]
            for i in bad[:5]:
                print("point", i, pts[i], "gpu", go[i], gs[i], ge[i], "oracle", ro[i], rs[i], re[i])
        assert ok, (it, h, w, kind, kw)
        if only >= 0:
            print("iteration", it, "ok")
            break
        it += 1; npts += n
print("lk fuzz ok: %d configurations, %d points in %.0f s" % (it, npts, time.time() - t0))
