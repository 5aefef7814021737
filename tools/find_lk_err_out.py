"""Seeded CPU search for inputs on which the LK tracker's error stage finds the FINAL position outside the next image
(status 0 after the Newton loop ended normally: `err_out` in the trace of tests/lk_ref.py), checked against
oracle/lk_oracle.c on the way.  Writes the cases with the most such points to tests/golden/lk_err_out_cases.npz.
usage: python tools/find_lk_err_out.py [cases] [seed] [keep]     (defaults 300 0 3; no GPU)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lk_ref
import oracle_lib as O
from test_lk_oracle import smooth_image

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
keep = int(sys.argv[3]) if len(sys.argv) > 3 else 3
found = []
for it in range(cases):
    h, w = (int(v) for v in rng.integers(24, 60, 2))
    a = rng.integers(0, 256, (h, w), dtype=np.uint8) if it % 2 == 0 else smooth_image(it, h, w)(0, 0)
    b = np.roll(a, tuple(int(v) for v in rng.integers(-2, 3, 2)), (0, 1))
    win = int(rng.integers(3, 12))
    pts = np.stack([rng.uniform(-win, w + win, 30), rng.uniform(-win, h + win, 30)], 1).astype(np.float32)
    kw = dict(win=win, max_level=int(rng.integers(0, 3)), max_iters=int(rng.integers(1, 40)),
              epsilon=float(rng.choice([0.0, 0.01, 0.03])))
    trace = []
    out, st, err, top = lk_ref.track(a, b, pts, trace=trace, **kw)
    ro, rs, re, rtop = O.lk_track(a, b, pts, **kw)
    assert top == rtop and np.array_equal(st, rs) and np.array_equal(out.view(np.uint32), ro.view(np.uint32)) and \
        np.array_equal(err.view(np.uint32), re.view(np.uint32)), (it, kw)
    hits = [r["point"] for r in trace if r["reason"] == "err_out"]
    if hits:
        print("case %d: %dx%d %s points %s" % (it, w, h, kw, hits))
        found.append((len(hits), it, a, b, pts, kw))
print("%d err_out points in %d of %d cases" % (sum(f[0] for f in found), len(found), cases))
found.sort(key=lambda f: (-f[0], f[1]))
z = {}
for k, (_, it, a, b, pts, kw) in enumerate(found[:keep]):
    z.update({"a%d" % k: a, "b%d" % k: b, "pts%d" % k: pts, "params%d" % k: np.float64(
        [kw["win"], kw["max_level"], kw["max_iters"], kw["epsilon"]])})
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "lk_err_out_cases.npz"), n=np.int32(min(keep, len(found))), **z)
