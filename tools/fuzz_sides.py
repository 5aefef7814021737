#!/usr/bin/env python3
"""Random-input parity campaign for the side paths: the draws of tests/side_random.py over an open index range, every
fetched array against the expected one bit for bit, all on one small context.
Usage: python tools/fuzz_sides.py [seconds] [seed] [--family f] [--only index]   (needs a GPU)
--family: one of side_random.FAMILIES (default: all of them in turn, each with the whole budget)
--only:   replay one draw verbosely on a fresh context
The first mismatch or error ends the run (nothing is caught and passed over) with the replay command.  The replay
command of the draw about to run also goes to stderr before every draw, so that a run that ends without a Python
error still names its draw; a progress line goes to stdout every 30 s."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import side_random as S  # noqa: E402

pkg = importlib.import_module("visual-odometry-gpu_amd")


def replay_command(family, seed, index):
    return "python tools/fuzz_sides.py 0 %d --family %s --only %d" % (seed, family, index)


def one(c, family, seed, index, verbose=False):
    d = S.draw(family, seed, index)
    if verbose:
        print("draw (%s, %d, %d): %s" % (family, seed, index, S.describe(family, d)), flush=True)
    got = S.run(family, c, d)
    try:
        S.compare(family, got, d)
    except AssertionError:
        print("MISMATCH at (%s, %d, %d): %s\nreplay: %s" % (family, seed, index, S.describe(family, d),
                                                            replay_command(family, seed, index)), flush=True)
        raise
    return S.elements(family, d)


def campaign(family, budget, seed):
    t0 = t_print = time.time()
    index = total = 0
    name = "elements"
    with S.context(pkg, family) as c:
        while time.time() - t0 < budget:
            if time.time() - t_print > 30:
                t_print = time.time()
                print("... %s: %d configurations, %d %s after %.0f s" % (family, index, total, name, t_print - t0),
                      flush=True)
            print("next: %s" % replay_command(family, seed, index), file=sys.stderr, flush=True)
            name, k = one(c, family, seed, index)
            total += k
            index += 1
    print("fuzz ok: %s: %d configurations, %d %s in %.0f s (seed %d)" % (family, index, total, name,
                                                                         time.time() - t0, seed), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seconds", nargs="?", type=float, default=60.0)
    ap.add_argument("seed", nargs="?", type=int, default=0)
    ap.add_argument("--family", choices=S.FAMILIES)
    ap.add_argument("--only", type=int)
    a = ap.parse_args()
    families = [a.family] if a.family else list(S.FAMILIES)
    if a.only is not None:
        for f in families:
            with S.context(pkg, f) as c:
                one(c, f, a.seed, a.only, verbose=True)
            print("draw (%s, %d, %d) ok" % (f, a.seed, a.only), flush=True)
        return
    for f in families:
        campaign(f, a.seconds, a.seed)


if __name__ == "__main__":
    main()
