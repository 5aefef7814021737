"""The Lucas-Kanade oracle (oracle/lk_oracle.c) against the numpy restatement written from the rules
(tests/lk_ref.py; DESIGN.md, LK rules 1-9): bit for bit on inputs whose trace shows that every way a level can end is
taken, and the restatement's fixed-point arithmetic against plain float64 within bounds derived from the rules, so
that the two cannot be exactly wrong in the same way.  No GPU."""
import collections

import numpy as np
import pytest

import lk_cases as K
import lk_ref
import oracle_lib as O
from lk_ref import np_scharr
from test_lk_oracle import smooth_image


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_oracle_equals_ref(name):
    prev, nxt, pts, kw = K.case(name)
    out, st, err, top, _ = K.ref(name)
    ro, rs, re, rtop = O.lk_track(prev, nxt, pts, **kw)
    assert top == rtop
    assert np.array_equal(st, rs), np.flatnonzero(st != rs)
    assert np.array_equal(bits(out), bits(ro)), np.flatnonzero((bits(out) != bits(ro)).any(1))
    assert np.array_equal(bits(err), bits(re)), np.flatnonzero(bits(err) != bits(re))
    return out, st, err, top


@pytest.mark.parametrize("name", [n for n in K.cases() if not n.startswith("win-")])
def test_oracle_equals_restatement(name):
    assert_oracle_equals_ref(name)


def test_oracle_equals_restatement_at_every_window_size():
    tops = {}
    for win in range(3, 32):
        out, st, err, top = assert_oracle_equals_ref("win-%d" % win)
        assert 10 <= st.sum() <= 40, (win, st.sum())  # points both kept and lost at every size
        tops[win] = top
    # 72 x 88 -> 36 x 44 -> 18 x 22: the second level exists while 18 > win
    assert tops == {win: 2 if win < 18 else 1 for win in range(3, 32)}


def test_non_finite_and_huge_coordinates_are_outside():
    """LK rule 9: NaN, or a floor that does not fit an int32, is out of bounds -- status 0, error 0, and the position
    handed down the levels unchanged in kind (NaN stays NaN)."""
    for k in range(len(K.SPECIAL_PARAMS)):
        pts = K.case("special-%d" % k)[2]
        out, st, err, top, trace = K.ref("special-%d" % k)
        odd = ~np.isfinite(pts).all(1) | (np.abs(pts) > 1e9).any(1)
        assert odd.sum() == 10 and not st[odd].any() and not err[odd].any()
        assert np.array_equal(np.isnan(out[odd]), np.isnan(pts[odd]))
        assert all(r["reason"] == "prev_out" for r in trace if odd[r["point"]])
        # the bounds of rule 3, from both sides: origin -win, w - 1 and the float just below w are inside (the level
        # gets as far as the template), the float just below -win, -win - 1 and w are outside
        last = {r["point"]: r["reason"] for r in trace if r["level"] == 0}
        assert all(last[i] != "prev_out" for i in (9, 10, 15, 16, 17, 18)), last
        assert all(last[i] == "prev_out" for i in (11, 12, 13, 14, 19, 20)), last
        assert st[:9].sum() >= 5


def test_every_way_a_level_ends_is_taken():
    """keeps the inputs honest: summed over the cases compared above, each reason occurs at least 5 times at level 0
    and at least 5 times above it"""
    n = collections.Counter()
    for name in K.cases():
        n.update((r["reason"], r["level"] > 0) for r in K.ref(name)[4])
    print(sorted(n.items()))
    for reason in ("prev_out", "min_eig", "eps", "osc", "iters", "next_out"):
        assert n[reason, False] >= 5 and n[reason, True] >= 5, (reason, n[reason, False], n[reason, True])


def test_error_stage_rejects_a_final_position_outside():
    """tests/golden/lk_err_out_cases.npz: the Newton loop ends on one of its own rules (status still 1), and the
    position it leaves, after the oscillation half-step if any, is outside the next image: status 0, error 0."""
    assert len(K.err_out_cases()) >= 2
    stops = collections.Counter()
    for name in K.err_out_cases():
        out, st, err, top = assert_oracle_equals_ref(name)
        hit = [r for r in K.ref(name)[4] if r["reason"] == "err_out"]
        assert hit, name
        for r in hit:
            assert r["level"] == 0 and r["stop"] in ("eps", "osc", "iters")
            assert st[r["point"]] == 0 and bits(err)[r["point"]] == 0
            stops[r["stop"]] += 1
    assert sum(stops.values()) >= 4, stops


def test_long_walks_within_one_level():
    """the inputs of test_lk_gpu.test_next_image_cache_is_refetched: the window's integer origin moves by more than
    2 px within a level, with its neighbourhood inside the image and over the border, at least 30 times each"""
    n = collections.Counter()
    for name in K.refetch_cases():
        assert_oracle_equals_ref(name)
        n.update(bool(r["inside"]) for r in K.ref(name)[4] if r["moved"] is not None and r["moved"] > 2)
    assert n[True] >= 30 and n[False] >= 30, n


# ---- fixed point against float64 ------------------------------------------------------------------------------
U = 2.0 ** -24                                # unit roundoff of float32
# Weights (rule 4), in units of 2^-14: a = x - floor(x) is exact in float32; 1 - a, the product of two factors and
# the product with 2^14 (exact) carry at most 3 roundings of relative size U on a value of at most 2^14, and rint
# adds at most 0.5: |dw| <= 0.5 + 3 U 2^14 for three weights.  The true weights sum to 2^14 exactly, so the fourth,
# which takes the remainder, is off by minus the sum of the other three errors: sum |dw| <= 2 * 3 * (0.5 + 3 U 2^14).
SUM_DW = 6 * (0.5 + 3 * U * 2 ** 14)          # 3.018
# iv = (sum w p + 256) >> 9 = floor(sum w p / 512 + 1/2), and sum w p = 2^14 I + sum dw p with p <= 255:
B_IV = 0.5 + SUM_DW * 255 / 512               # 2.003 on iv - 32 I
# ix = (sum w d + 8192) >> 14 with Scharr |d| <= 16 * 255 = 4080:
B_IG = 0.5 + SUM_DW * 4080 / 16384            # 1.252 on ix - Dx, iy - Dy


def bilinear64(a, x0, y0, fx, fy, win):
    """plain float64 bilinear interpolation of the extended map `a` (whose [0, 0] is image position (x0, y0)) at the
    win x win positions (fx + i, fy + j)"""
    ix, iy = int(np.floor(fx)), int(np.floor(fy))
    ax, ay = fx - ix, fy - iy
    s = a[iy - y0:iy - y0 + win + 1, ix - x0:ix - x0 + win + 1].astype(np.float64)
    return (1 - ax) * (1 - ay) * s[:-1, :-1] + ax * (1 - ay) * s[:-1, 1:] + (1 - ax) * ay * s[1:, :-1] + \
        ax * ay * s[1:, 1:]


def test_fixed_point_template_against_float64():
    """The restatement is exact, so it could be exactly wrong like the oracle; this anchors both.  On 40 frames of
    40 x 48 (noise and texture alternating), a random window size and 50 random sub-pixel window origins in
    [-win, w) x [-win, h) per frame: the template the trace records against float64 bilinear interpolation of the
    REFLECT_101-extended image and of the zero-extended Scharr maps, within bounds derived above from the rules
    (B_IV = 2.003 for iv against 32 I, B_IG = 1.252 for ix, iy), not fitted to any output.  Then the gradient
    matrix against the float64 sums of the float64 gradients, and min_eig against numpy.linalg.eigvalsh."""
    h, w = 40, 48
    rng = np.random.default_rng(2024)
    worst = collections.defaultdict(float)
    for k in range(40):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8) if k % 2 == 0 else smooth_image(100 + k, h, w)(0, 0)
        win = int(rng.integers(3, 32))
        half = np.float32(win - 1) * np.float32(0.5)
        origin = np.stack([rng.uniform(-win, w, 50), rng.uniform(-win, h, 50)], 1)
        pts = (origin + float(half)).astype(np.float32)
        trace = []
        lk_ref.track(img, img, pts, win=win, max_level=0, max_iters=0, trace=trace)
        pad = win + 1  # <= 32 < h, w: one reflection, which numpy's own "reflect" (REFLECT_101) does
        ext = np.pad(img.astype(np.int64), pad, mode="reflect")
        d = np_scharr(img).astype(np.int64)
        extx, exty = np.pad(d[..., 0], pad), np.pad(d[..., 1], pad)
        assert len(trace) == 50
        for r in trace:
            # rule 3: the window's real-valued origin is the float32 difference position - half
            fx, fy = (float(v - half) for v in pts[r["point"]])
            if not (np.floor(fx) >= -win and np.floor(fy) >= -win and np.floor(fx) < w and np.floor(fy) < h):
                assert r["reason"] == "prev_out"  # (the float32 sum origin + half rounded up to the bound)
                continue
            assert r["origin"] == (int(np.floor(fx)), int(np.floor(fy)))
            i64 = bilinear64(ext, -pad, -pad, fx, fy, win)
            gx, gy = bilinear64(extx, -pad, -pad, fx, fy, win), bilinear64(exty, -pad, -pad, fx, fy, win)
            e_iv, e_ix, e_iy = (np.abs(r["iv"] - 32 * i64).max(), np.abs(r["ix"] - gx).max(),
                                np.abs(r["iy"] - gy).max())
            for key, v in (("iv", e_iv), ("ix", e_ix), ("iy", e_iy)):
                worst[key] = max(worst[key], v)
            assert e_iv <= B_IV and e_ix <= B_IG and e_iy <= B_IG, (k, r["point"], e_iv, e_ix, e_iy)
            # Rule 5: A = float32(exact sum of products) * 2^-20.  With |ix - gx|, |iy - gy| <= B = B_IG,
            # |ix ix - gx gx| <= B (2 |gx| + B) and |ix iy - gx gy| <= B (|gx| + |gy| + B) per pixel; the conversion
            # to float32 adds a relative U and the scaling is exact.
            B = B_IG
            for key, got, want, slack in (("A11", r["A11"], gx * gx, B * (2 * np.abs(gx) + B)),
                                          ("A12", r["A12"], gx * gy, B * (np.abs(gx) + np.abs(gy) + B)),
                                          ("A22", r["A22"], gy * gy, B * (2 * np.abs(gy) + B))):
                bound = slack.sum() * 2.0 ** -20 + U * abs(float(got))
                assert abs(float(got) - want.sum() * 2.0 ** -20) <= bound, (k, r["point"], key)
            # min_eig = ((A22 + A11) - sqrt((A11 - A22)^2 + 4 A12 A12)) / (2 win^2) in float32, one rounding per
            # operation.  With t = A11 + A22 >= r = the root: the sum has relative error U; A11 - A22 has U, its
            # square 3 U, (4 A12) A12 has U, their sum 4 U, the root 2 U + U = 3 U; so the difference is off by at
            # most U t + 3 U r + U |t - r| <= 5 U t, and the division (2 win^2 is exact) adds U: 6 U t / (2 win^2),
            # asserted with 8 for the second-order terms.
            A = np.array([[r["A11"], r["A12"]], [r["A12"], r["A22"]]], np.float64)
            lam = 2 * np.linalg.eigvalsh(A)[0] / (2 * win * win)  # t - r is twice the smaller eigenvalue
            bound = 8 * U * (A[0, 0] + A[1, 1]) / (2 * win * win)
            assert abs(float(r["min_eig"]) - lam) <= bound, (k, r["point"], float(r["min_eig"]), lam)
    print({key: round(float(v), 3) for key, v in worst.items()})
    assert worst["iv"] > 0.25 and worst["ix"] > 0.25  # sub-pixel positions were seen: the descale alone rounds by up to 0.5
