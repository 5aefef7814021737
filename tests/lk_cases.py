"""The small Lucas-Kanade inputs shared by tests/test_lk_ref.py (oracle against the numpy restatement, no GPU) and
the GPU tests (tests/test_lk_gpu.py, tests/test_lk_windows.py), and the restatement's result on each of them,
computed once per process and handed out read-only.  A case is (prev, next, pts, kw)."""
import functools
import os

import numpy as np

import lk_ref
from test_lk_oracle import smooth_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWEEP = [(21, 3, 30, 0.01), (5, 0, 10, 0.03), (31, 5, 3, 0.001), (9, 2, 100, 0.0), (15, 7, 0, 0.01), (3, 1, 30, 0.01)]
SPECIAL_PARAMS = [dict(win=21, max_level=3), dict(win=3, max_level=3),
                  dict(win=5, max_level=2, max_iters=100, epsilon=0.0)]
REFETCH_PARAMS = [dict(win=21, max_level=0), dict(win=9, max_level=0),
                  dict(win=13, max_level=1, max_iters=60, epsilon=0.0)]


def kwargs(win, max_level, max_iters, eps):
    return dict(win=win, max_level=max_level, max_iters=max_iters, epsilon=eps)


def sweep_points(win, n):
    """the point recipe of test_lk_gpu.test_parameter_sweep_with_border_points with n random points"""
    rng = np.random.default_rng(win)
    return np.concatenate([
        np.stack([rng.uniform(-30, 240, n), rng.uniform(-30, 180, n)], 1),
        np.float32([[0, 0], [210, 149], [0.5, 148.5], [105.25, 74.75], [-21, 10], [211, 75], [1e4, 1e4], [-1e4, 3]]),
    ]).astype(np.float32)


def special_points(win, w, h):
    """Positions at which a rule changes its answer: exact and half pixels, weights that round to 16384 / 0, signed
    zero and a denormal, the corners, window origins (position - (win - 1) / 2, floored) on both sides of each bound
    of [-win, w) x [-win, h), and the non-finite and out-of-int32 coordinates."""
    f = np.float32
    half = f(win - 1) * f(0.5)
    mx, my = f(w // 2) + f(0.25), f(h // 2) + f(0.75)
    nan, inf = f(np.nan), f(np.inf)
    below = lambda v: np.nextafter(f(v), f(-np.inf))
    p = [(20, 17), (20.5, 17.5), (20.5, 17), (np.nextafter(f(11), f(0)), 17), (20, np.nextafter(f(11), f(0))),
         (-0.0, -0.0), (1e-40, 1e-40), (w - 1, h - 1), (w, h)]
    for lo in (f(-win), below(-win), f(-win - 1)):       # origin -win, just below it, -win - 1
        p += [(lo + half, my), (mx, lo + half)]
    # origin w - 1, just below w (the position is the coarser float there: step it, not the origin), w
    for hx, hy in ((f(w - 1) + half, f(h - 1) + half), (below(f(w) + half), below(f(h) + half)), (w + half, h + half)):
        p += [(hx, my), (mx, hy)]
    p += [(nan, my), (mx, nan), (nan, nan), (inf, my), (mx, -inf), (3e9, my), (mx, -3e9), (1e30, my),
          (2147483520.0, my), (mx, -2147483648.0)]
    return np.array(p, np.float32)


@functools.lru_cache(None)
def cases():
    """name -> (prev, next, pts, kw): every input of test_lk_ref's oracle-against-restatement comparison"""
    c = {}
    f = smooth_image(5, 150, 211)
    prev, nxt = f(0, 0), f(-2.4, 1.7)
    for t in SWEEP:
        c["sweep-%d" % t[0]] = (prev, nxt, sweep_points(t[0], 120), kwargs(*t))
    rng = np.random.default_rng(0)  # test_lk_gpu.test_noise_and_flat_images, its first 150 points
    a = rng.integers(0, 256, (97, 131), dtype=np.uint8)
    pts = np.stack([rng.uniform(0, 131, 200), rng.uniform(0, 97, 200)], 1).astype(np.float32)[:150]
    c["noise"] = (a, np.roll(a, (1, 2), (0, 1)), pts, {})
    flat = np.full((97, 131), 200, np.uint8)
    c["flat"] = (flat, flat, pts, {})
    z = np.load(os.path.join(GOLDEN, "lk_min_eig_case.npz"))
    c["min-eig"] = (z["a"], z["b"], z["pts"], kwargs(14, 0, 31, 0.0))
    f = smooth_image(7, 72, 88)
    prev, nxt = f(0, 0), f(-1.3, 0.6)
    rng = np.random.default_rng(7)
    pts = np.stack([rng.uniform(-8, 96, 40), rng.uniform(-8, 80, 40)], 1).astype(np.float32)
    for win in range(3, 32):
        c["win-%d" % win] = (prev, nxt, pts, dict(win=win, max_level=2))
    f = smooth_image(7, 48, 56)
    prev, nxt = f(0, 0), f(-1.3, 0.6)
    for k, kw in enumerate(SPECIAL_PARAMS):
        c["special-%d" % k] = (prev, nxt, special_points(kw["win"], 56, 48), kw)
    for v in c.values():
        for a in v[:3]:
            a.setflags(write=False)
    return c


@functools.lru_cache(None)
def err_out_cases():
    """tests/golden/lk_err_out_cases.npz (tools/find_lk_err_out.py): inputs whose error stage finds the final
    position outside the next image"""
    z = np.load(os.path.join(GOLDEN, "lk_err_out_cases.npz"))
    out = {}
    for k in range(int(z["n"])):
        win, max_level, max_iters, eps = z["params%d" % k]
        out["err-out-%d" % k] = (z["a%d" % k], z["b%d" % k], z["pts%d" % k],
                                 kwargs(int(win), int(max_level), int(max_iters), float(eps)))
    return out


@functools.lru_cache(None)
def refetch_cases():
    """a shift the Newton steps have to walk (4.6, 3.3 px) without a pyramid to absorb it: the window's integer origin
    leaves the margin of the kernel's LDS cache of the next image"""
    f = smooth_image(11, 64, 80)
    prev, nxt = f(0, 0), f(-4.6, 3.3)
    rng = np.random.default_rng(11)
    pts = np.stack([rng.uniform(-6, 86, 80), rng.uniform(-6, 70, 80)], 1).astype(np.float32)
    return {"refetch-%d" % k: (prev, nxt, pts, kw) for k, kw in enumerate(REFETCH_PARAMS)}


def case(name):
    for group in (cases, err_out_cases, refetch_cases):
        if name in group():
            return group()[name]
    raise KeyError(name)


@functools.lru_cache(None)
def ref(name):
    """(next_pts, status, err, top, trace) of lk_ref.track on case(name); the arrays are read-only"""
    prev, nxt, pts, kw = case(name)
    trace = []
    out, st, err, top = lk_ref.track(prev, nxt, pts, trace=trace, **kw)
    for a in (out, st, err):
        a.setflags(write=False)
    return out, st, err, top, trace
