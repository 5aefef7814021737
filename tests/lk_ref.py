"""Numpy restatement of the library's pyramidal Lucas-Kanade tracker (the LK rules 1-9): what
orbx_lk_track and oracle/lk_oracle.c compute, bit for bit.  Written from the rules, not from either text, and laid
out differently on purpose: every level is an int64 array extended by REFLECT_101 (the derivative maps by zeros) so
that a window is a plain slice, the whole win x win window is one array expression per step, integer sums are Python
ints, every float32 operation is ONE numpy float32 operation (rounded once; numpy never contracts), and the two stop
rules are evaluated in Python floats (binary64).

track(..., trace=[]) appends one record per (point, level): see `track`."""
import numpy as np

F = np.float32
W_ONE = 1 << 14                   # the bilinear weights are 14-bit fixed point
FLT_SCALE = F(1.0 / (1 << 20))    # window sums -> float
MIN_EIG = F(1e-4)
FLT_EPS = F(2.0 ** -23)


def np_pyr_down(img):
    h, w = img.shape
    k = np.array([1, 4, 6, 4, 1])
    p = np.pad(img.astype(np.int64), 2, mode="reflect")
    dh, dw = (h + 1) // 2, (w + 1) // 2
    out = np.zeros((dh, dw), np.int64)
    for i in range(5):
        for j in range(5):
            out += k[i] * k[j] * p[i:i + 2 * dh:2, j:j + 2 * dw:2][:dh, :dw]
    return ((out + 128) >> 8).astype(np.uint8)


def np_scharr(img):
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    h, w = img.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    dx = 3 * (s(-1, 1) - s(-1, -1)) + 10 * (s(0, 1) - s(0, -1)) + 3 * (s(1, 1) - s(1, -1))
    dy = 3 * (s(1, -1) - s(-1, -1)) + 10 * (s(1, 0) - s(-1, 0)) + 3 * (s(1, 1) - s(-1, 1))
    return np.stack([dx, dy], -1).astype(np.int16)


def reflect_index(lo, hi, n):
    """REFLECT_101 source index of every position in [lo, hi) of an axis of n samples (period 2n - 2)"""
    if n == 1:
        return np.zeros(hi - lo, np.int64)
    m = np.arange(lo, hi) % (2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


class Level:
    """One pyramid level, extended by `pad` on every side: img by reflection, dx / dy (if wanted) by zeros"""

    def __init__(self, img, pad, with_deriv):
        self.h, self.w = img.shape
        self.pad = pad
        ys, xs = reflect_index(-pad, self.h + pad, self.h), reflect_index(-pad, self.w + pad, self.w)
        self.img = img.astype(np.int64)[ys[:, None], xs[None, :]]
        if with_deriv:
            d = np_scharr(img).astype(np.int64)
            self.dx, self.dy = (np.pad(d[..., c], pad) for c in (0, 1))

    def window(self, a, x, y, n):
        """a[y .. y + n, x .. x + n] in image coordinates: the (n + 1)^2 samples an n x n bilinear window reads"""
        return a[y + self.pad:y + self.pad + n + 1, x + self.pad:x + self.pad + n + 1]


def pyramid(img, win, max_level, with_deriv):
    """Rule 1: level l + 1 = pyrDown(level l), as long as it is larger than the window in both directions"""
    levels = [np.ascontiguousarray(img, np.uint8)]
    while len(levels) <= max_level:
        h, w = levels[-1].shape
        if (w + 1) // 2 <= win or (h + 1) // 2 <= win:
            break
        levels.append(np_pyr_down(levels[-1]))
    return [Level(a, win + 1, with_deriv) for a in levels]


def floor_in(v, n, win):
    """Rules 3 and 9: the integer origin floor(v) of a window along an axis of n samples, or None if the window is
    outside: v is NaN, floor(v) does not fit an int32, or floor(v) is not in [-win, n)."""
    f = np.floor(v)
    if not (f >= -2147483648.0 and f < 2147483648.0):  # false for NaN
        return None
    i = int(f)
    return i if -win <= i < n else None


def weights(a, b):
    """Rule 4: three weights rounded half to even, the fourth takes the remainder"""
    one, s = F(1), F(W_ONE)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, W_ONE - w00 - w01 - w10


def bilinear(s, w, bits):
    """the window of the (n + 1)^2 samples s under the weights w, descaled by `bits` with rounding"""
    v = s[:-1, :-1] * w[0] + s[:-1, 1:] * w[1] + s[1:, :-1] * w[2] + s[1:, 1:] * w[3]
    return (v + (1 << (bits - 1))) >> bits


def to_f32(total):
    """an exact integer sum as float32: through binary64 (exact below 2^53), then rounded once"""
    return F(float(int(total))) * FLT_SCALE


def track(prev, next, pts, win=21, max_level=3, max_iters=30, epsilon=0.01, trace=None):
    """Returns (next_pts, status, err, top).  trace (a list) receives one dict per (point, level):
    point, level, reason (prev_out | min_eig | next_out | eps | osc | iters | err_out; err_out replaces the reason the
    Newton loop ended with, which stays in `stop`), A11, A12, A22, min_eig, iv / ix / iy (win x win int64), origin
    (x, y) and weights of the template, moved (largest Chebyshev distance of a next-image window origin of this
    level, the error stage's included, from the first one) and inside (whether the first origin's (win + 5)^2
    neighbourhood, from origin - 2, lies inside the level).  Fields a level did not reach are None."""
    if not (3 <= win <= 31 and 0 <= max_level <= 7):
        raise ValueError("win / max_level")
    max_iters = min(max(int(max_iters), 0), 100)
    eps2 = min(max(float(epsilon), 0.0), 10.0) ** 2
    P, N = pyramid(prev, win, max_level, True), pyramid(next, win, max_level, False)
    top = len(P) - 1
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    out, status, err = np.zeros((n, 2), np.float32), np.ones(n, np.uint8), np.zeros(n, np.float32)
    half = F(win - 1) * F(0.5)
    for i in range(n):
        ox = oy = F(0)
        for level in range(top, -1, -1):
            I, J = P[level], N[level]
            rec = dict(point=i, level=level, reason=None, stop=None, A11=None, A12=None, A22=None, min_eig=None,
                       iv=None, ix=None, iy=None, origin=None, weights=None, moved=None, inside=None)
            if trace is not None:
                trace.append(rec)
            sc = F(1.0 / (1 << level))
            px, py = pts[i, 0] * sc, pts[i, 1] * sc
            # rule 2: the start is the point itself at the top, twice the result of the level above below it;
            # it is the level's result if the level is skipped
            ox, oy = (px, py) if level == top else (ox * F(2), oy * F(2))
            px, py = px - half, py - half
            ipx, ipy = floor_in(px, I.w, win), floor_in(py, I.h, win)
            if ipx is None or ipy is None:
                rec["reason"] = "prev_out"
                if level == 0:
                    status[i], err[i] = 0, 0
                continue
            # rule 5: the template and its gradient matrix
            wi = weights(px - F(ipx), py - F(ipy))
            iv = bilinear(I.window(I.img, ipx, ipy, win), wi, 9)
            ix = bilinear(I.window(I.dx, ipx, ipy, win), wi, 14)
            iy = bilinear(I.window(I.dy, ipx, ipy, win), wi, 14)
            A11, A12, A22 = to_f32((ix * ix).sum()), to_f32((ix * iy).sum()), to_f32((iy * iy).sum())
            D = A11 * A22 - A12 * A12
            dif = A11 - A22
            min_eig = ((A22 + A11) - np.sqrt(dif * dif + F(4) * A12 * A12)) / F(2 * win * win)
            rec.update(A11=A11, A12=A12, A22=A22, min_eig=min_eig, iv=iv, ix=ix, iy=iy, origin=(ipx, ipy), weights=wi)
            if min_eig < MIN_EIG or D < FLT_EPS:
                rec["reason"] = "min_eig"
                if level == 0:
                    status[i] = 0
                continue
            D = F(1) / D
            nx, ny = ox - half, oy - half
            pdx = pdy = F(0)
            first, moved = None, 0

            def next_window(x, y):
                """the window at (x, y) of the next image minus the template, or None if it is outside"""
                nonlocal first, moved
                inx, iny = floor_in(x, J.w, win), floor_in(y, J.h, win)
                if inx is None or iny is None:
                    return None
                if first is None:
                    first = (inx, iny)
                    rec["inside"] = (inx >= 2 and iny >= 2 and inx + win + 3 <= J.w and iny + win + 3 <= J.h)
                moved = max(moved, abs(inx - first[0]), abs(iny - first[1]))
                rec["moved"] = moved
                return bilinear(J.window(J.img, inx, iny, win), weights(x - F(inx), y - F(iny)), 9) - iv

            # rules 6 and 7: Newton steps; position updated, then epsilon, then oscillation
            stop = "iters"
            for j in range(max_iters):
                diff = next_window(nx, ny)
                if diff is None:
                    stop = "next_out"
                    if level == 0:
                        status[i] = 0
                    break
                b1, b2 = to_f32((diff * ix).sum()), to_f32((diff * iy).sum())
                dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                nx, ny = nx + dx, ny + dy
                ox, oy = nx + half, ny + half
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                    stop = "eps"
                    break
                if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                    ox, oy = ox - dx * F(0.5), oy - dy * F(0.5)
                    stop = "osc"
                    break
                pdx, pdy = dx, dy
            rec["reason"] = rec["stop"] = stop
            # rule 8: the error at level 0, at the final position
            if level == 0 and status[i]:
                diff = next_window(ox - half, oy - half)
                if diff is None:
                    rec["reason"] = "err_out"
                    status[i] = 0
                else:
                    err[i] = F(float(int(np.abs(diff).sum()))) * (F(1) / F(32 * win * win))
        out[i] = ox, oy
    return out, status, err, top
