"""Every accepted detector parameter through the launch sequences that only large batches reach: the top-rows-first
two-pass pyramid with its uneven first cut and early band, the FAST early exit over stale mask words, the selection
kernel with one workgroup per frame (256 frames and more) and graph replay on two lanes.  Every other test that reaches
them runs the benchmark's parameters (arc length 9, nms_window 3, threshold 20 or 12, patch_size 31); here ONE parameter
at a time moves from that base to each value validate_params accepts and the fuzzer draws, at the smallest shape that
runs two passes -- the one of test_fast_first_split.py: 320 x 160, 4 levels, scale 1.2, 200 features, blur on every
level --, plus two combined cases and the launch sequences that are not fused.

Frames: the seven dots frames and the noise frame of test_fast_first_split.py, a constant frame (no survivor at any
threshold: a score of 0 is no keypoint), a frame with dots below row 90 only (its level-0 cap fills below the first
pass or never) and a frame of random 4 x 4 cells of 40 / 220 (dense corners: its caps fill inside the first pass where
one level holds every feature, at scale 2.7 and with 1000 features, where no dots frame's do), tiled to the smallest
multiple of eleven frames that gives the fused pyramid kernel 4096 strips (264 for the base plan's 16 strips per
frame; more for fewer or coarser levels).

CPU half (not gpu): a CONDITION per case, from the oracle's fill rows F = row of the cap-th survivor + 1 per (frame,
level): some (frame, level) fills inside the first pass of a level that has a second one -- so the second pass must
skip strips and FAST units must exit --, and some fills below it or never -- so the second pass must also work.  Where
a case cannot meet it (nfeatures 0: every cap is 0 and holds before the first row) it asserts exactly that instead.

GPU half: run() below, with both FAST kernels; bit for bit against the oracle (the row-major reference of
tools/fuzz_parity.py for select_mode 1)."""
import concurrent.futures as cf
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O
import test_fast_first_split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

W, H = S.W, S.H
BASE = dict(S.PK, scale_factor=1.2, harris_window=7, harris_k=0.04)
assert (BASE["nfeatures"], BASE["nlevels"], BASE["blur_levels"], BASE["blur_kind"]) == (200, 4, 2, 0)

CASES = {"base": {}}
for _name, _values in (("nms_window", (0, 5, 7)), ("n", (1, 5, 12, 16)), ("threshold", (0, 1, 60, 120)),
                       ("patch_size", (1, 9, 15, 41)), ("harris_window", (1, 3, 5, 9, 15)), ("harris_k", (0.0, 0.06)),
                       ("nfeatures", (0, 7, 1000)), ("select_mode", (1,)), ("nlevels", (1,))):
    for _v in _values:
        CASES["%s=%s" % (_name, _v)] = {_name: _v}
CASES["scale_factor=1.5,nlevels=3"] = dict(scale_factor=1.5, nlevels=3)
CASES["scale_factor=2.7,nlevels=3"] = dict(scale_factor=2.7, nlevels=3)
CASES["combined-wide"] = dict(nms_window=7, n=12, threshold=35, patch_size=41, harris_window=15)
CASES["combined-loose"] = dict(nms_window=0, threshold=0, n=1)
# the launch sequence that is not fused: pyramid, then the stand-alone blur, then one FAST launch
CASES["blur_levels=1"] = dict(blur_levels=1)
CASES["blur_kind=1"] = dict(blur_levels=2, blur_kind=1)

_cache = {}


def frames():
    """the eight frames of test_fast_first_split.py, a constant one, one with dots below row 90 only, a dense one"""
    if "frames" not in _cache:
        low = S.dots(31, 1.0)
        low[:90] = 60
        cells = np.random.default_rng(5).integers(0, 2, (H // 4, W // 4))
        dense = (40 + 180 * np.kron(cells, np.ones((4, 4), np.int64))).astype(np.uint8)
        _cache["frames"] = np.concatenate([S.data()[0], np.full((1, H, W), 60, np.uint8), low[None], dense[None]])
    return _cache["frames"]


CONSTANT = 8  # index of the constant frame
NOISE = 7     # ... of the uniform noise of test_fast_first_split.py (128 +- 60)
# Every frame but the constant one has keypoints on two levels or more wherever threshold <= 60 -- but for the noise
# frame in these cases: uniform noise has no arc of 16 ring pixels and hardly one of 12 on one side of its centre, and
# few pixels 60 grey levels above or below nine of their neighbours in a row
NOISE_SPARSE = ("n=16", "threshold=60", "combined-wide")


def params(case):
    kw = dict(BASE, **CASES[case])
    mode = kw.pop("select_mode", 0)
    return kw, mode


def fused(kw):
    return kw["blur_levels"] == 2 and kw["blur_kind"] == 0


def geometry(kw):
    """per level, restated from csrc/orbx_plan.h: width, height, rows of the first pass of two default tile rows
    (make_bandmap: balanced tile rows of at most 49 - 2 R), whether the level has a second pass
    (pyrblur_first_pass_rows: more than two tile rows, and rows below the first pass + ORBX_TOP_MARGIN), and the
    strips of the fused pyramid kernel (build_pyrblur_tiles: 62 dwords per strip, bands of at most 58 rows)"""
    out = []
    th = 49 - 2 * (kw["nms_window"] // 2)
    for l in range(kw["nlevels"]):
        w, h = O.level_size(W, H, kw["scale_factor"], l)
        ty = -(-h // th)
        depth = 2 * -(-h // ty)
        dw = (w + 3) // 4
        strips = (1 if dw <= 64 else (dw - 2 + 61) // 62) * -(-h // 58)
        out.append(dict(w=w, h=h, depth=depth, second=ty > 2 and depth + 21 < h, strips=strips))
    return out


def batch_size(kw):
    """two passes need n x (strips per frame) >= 4096: the smallest multiple of the frame set, at least 256 frames"""
    per_frame = sum(g["strips"] for g in geometry(kw))
    need = max(256, -(-4096 // per_frame))
    k = len(frames())
    return -(-need // k) * k


def caps(kw, mode):
    if mode == 1 and kw["nlevels"] == 1:
        return [kw["nfeatures"]]
    q = [max(O.level_quota(kw["nfeatures"], kw["scale_factor"], kw["nlevels"], l), 0) for l in range(kw["nlevels"])]
    return [v if mode == 1 else 2 * v for v in q]


def references(case):
    """the oracle's results for the eleven frames, and the fill rows [frame][level] (computed once per case)"""
    if case not in _cache:
        kw, mode = params(case)
        fr = frames()
        op = O.gpu_params(**kw)
        O.lib()
        cap = caps(kw, mode)

        def one(f):
            ref = O.detect_and_compute_gpu(f, op) if mode == 0 else F.rowmajor_ref(f, kw)
            fill = []
            for l in range(kw["nlevels"]):
                lvl = O.build_level(f, op, l)
                k = O.fast_detect(lvl, kw["threshold"], kw["n"], kw["nms_window"], cap[l]) if cap[l] > 0 else []
                # (a cap of 0 holds before the first row: the kernels' test is survivors >= cap)
                fill.append(0 if cap[l] == 0 else int(k[-1][1]) + 1 if len(k) == cap[l] else 10 ** 6)
            return ref, fill

        with cf.ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL
            res = list(ex.map(one, fr))
        _cache[case] = ([r for r, _ in res], np.array([f for _, f in res]))
    return _cache[case]


def fills(case):
    """(frame, level)s of the levels with a second pass that fill inside the first pass / below it or never"""
    kw, _ = params(case)
    _, fill = references(case)
    inside = below = 0
    for l, g in enumerate(geometry(kw)):
        if g["second"]:
            inside += int((fill[:, l] <= g["depth"]).sum())
            below += int((fill[:, l] > g["depth"]).sum())
    return inside, below


def forced_cuts(case):
    """rows of tile row 0 per level: the median fill row of the frames that fill inside the first pass (the library
    takes the nearest cut its kernel can run), so that some frames leave tile row 1 and skip the early band"""
    kw, _ = params(case)
    _, fill = references(case)
    cuts = []
    for l, g in enumerate(geometry(kw)):
        v = sorted(int(x) for x in fill[:, l] if 0 < x < g["depth"])
        cuts.append(v[len(v) // 2] if g["second"] and v else 0)
    return cuts


# ---- CPU half -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_the_case_fills_inside_and_below_the_first_pass(case):
    kw, mode = params(case)
    refs, fill = references(case)
    geo = geometry(kw)
    n = batch_size(kw)
    assert n >= 256 and n * sum(g["strips"] for g in geo) >= 4096 and n % len(frames()) == 0
    assert any(g["second"] for g in geo)
    inside, below = fills(case)
    print("%s: batch %d, caps %s, first pass %s, fill rows\n%s" % (case, n, caps(kw, mode), [g["depth"] for g in geo], fill))
    if kw["nfeatures"] == 0:
        assert not any(caps(kw, mode)) and below == 0 and inside > 0 and all(len(r["kps"]) == 0 for r in refs)
    else:
        assert inside > 0, "no (frame, level) fills inside the first pass: the second pass skips nothing"
        assert below > 0, "every (frame, level) fills inside the first pass: the second pass has nothing to do"
    if kw["nfeatures"] == 1000:
        # the case is there for the spread selection kernels (more than one candidate per thread of k_level_select: a
        # cap above 512); of the first eight frames no level with a second pass fills inside its first pass
        assert max(caps(kw, mode)) > 512
        assert all(fill[:8, l].min() > g["depth"] for l, g in enumerate(geo) if g["second"])
    assert (fill[CONSTANT] == (0 if kw["nfeatures"] == 0 else 10 ** 6)).all() and len(refs[CONSTANT]["kps"]) == 0
    if kw["threshold"] <= 60 and kw["nfeatures"] > 0:
        for i, r in enumerate(refs):
            levels = len(np.unique(r["levels"]))
            if i == NOISE and case in NOISE_SPARSE:
                # (stated, so that the list cannot grow unnoticed: the frame has keypoints on one level or on none)
                assert levels < 2, (i, np.bincount(r["levels"]))
            elif i != CONSTANT:
                assert levels >= min(2, kw["nlevels"]), (i, np.bincount(r["levels"]))


def test_the_base_shape_is_the_one_of_the_first_split_tests():
    geo = geometry(BASE)
    assert sum(g["strips"] for g in geo) == 16 and batch_size(BASE) == 264
    assert [g["depth"] for g in geo] == [d for _, _, d in S.level_rows()]
    assert [g["second"] for g in geo] == [True, True, True, False]


# ---- GPU half -------------------------------------------------------------------------------------------------------------
def compare(res, refs, n, tag):
    for i in range(n):
        m = int(res["counts"][i])
        got = dict(count=m, **{k: res[k][i, :m] for k in ("kps", "kps_level", "levels", "angles", "responses", "desc")})
        F.check(got, refs[i % len(refs)], (tag, i))


def run(pkg, monkeypatch, case, impl):
    """1. a pipelined context (two lanes, one graph per lane), the first pass cut at forced_cuts();  2. the eleven frames;
    3. the pools filled with 0xFF;  4. the eleven frames four times: both lanes replay their graphs;  5. the large batch
    three times, the pools filled again before the second (after two of them the scheduler may re-tile);  6. the large
    batch with the two passes whenever eligible (equal tile rows, no band) and in one pass;  7. the large batch with
    the compact record written to the host by the describe kernel.  Every batch equals the oracle."""
    import torch

    kw, mode = params(case)
    refs, _ = references(case)
    fr = frames()
    k, n = len(fr), batch_size(kw)
    monkeypatch.setenv("ORBX_FAST_IMPL", impl)
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:" + ",".join(str(c) for c in forced_cuts(case)))
    d_small = torch.from_numpy(fr).cuda()
    d_big = torch.from_numpy(np.tile(fr, (n // k, 1, 1))).cuda()
    torch.cuda.synchronize()
    eligible = fused(kw)
    inside, _ = fills(case)

    def two_passes_ran(c, what):
        produced, total = c.pyramid_pixel_counts()
        worked, units = c.fast_tile_counts()
        print("%s impl %s %s: %d of %d pyramid pixels, %d of %d FAST units" % (case, impl, what, produced, total, worked, units))
        if not eligible:
            assert produced == total, (what, produced, total)
        else:
            assert inside > 0  # (the CPU half's condition)
            assert produced < total, (what, produced, total)
            assert worked < units, (what, worked, units)

    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=n, select_mode=mode, **kw)
    with pkg.Context(p) as c:
        c.set_pipelined_batches(True)
        cap = max(c.plan(W, H)["out_capacity"], 1)
        c.batch_device(d_small.data_ptr(), k, W, H)  # (sets the plan: the fill below reaches the pyramid's pixels)
        compare(c.batch_fetch(0, k, cap), refs, k, (case, impl, "first"))
        c.debug_fill_pools(0xFF)
        for i in range(4):
            c.batch_device(d_small.data_ptr(), k, W, H)
            compare(c.batch_fetch(0, k, cap), refs, k, (case, impl, "small", i))
        for i in range(3):
            if i == 1:
                c.debug_fill_pools(0xFF)
            c.batch_device(d_big.data_ptr(), n, W, H)
            compare(c.batch_fetch(0, n, cap), refs, n, (case, impl, "large", i))
            if i == 0:
                two_passes_ran(c, "forced cut")
        c.set_top_rows_first(1)
        c.batch_device(d_big.data_ptr(), n, W, H)
        compare(c.batch_fetch(0, n, cap), refs, n, (case, impl, "two passes"))
        two_passes_ran(c, "whenever eligible")
        c.set_top_rows_first(0)
        c.batch_device(d_big.data_ptr(), n, W, H)
        compare(c.batch_fetch(0, n, cap), refs, n, (case, impl, "one pass"))
        produced, total = c.pyramid_pixel_counts()
        assert produced == total
        c.set_top_rows_first(2)
        c.set_host_results(True)
        c.batch_device(d_big.data_ptr(), n, W, H)
        hv = F.host_record(c)
        r = c.batch_fetch(0, n, cap)
        compare(r, refs, n, (case, impl, "host results"))
        for i in range(n):  # what the kernel wrote into the pinned mirror == what the copy of the block delivers
            m = int(r["counts"][i])
            assert int(hv["counts"][i]) == m, (case, impl, i)
            if m == 0:
                continue
            assert np.array_equal(hv["kps16"][i, :m].astype(np.int32), r["kps"][i, :m]), (case, impl, i)
            assert np.array_equal(hv["angles"][i, :m].view(np.uint32), r["angles"][i, :m].view(np.uint32)), (case, impl, i)
            assert np.array_equal(hv["desc"][i, :m], r["desc"][i, :m]), (case, impl, i)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["4", "3"], ids=["fast-stream", "fast-tiles"])
@pytest.mark.parametrize("case", list(CASES))
def test_large_batches_equal_the_oracle(pkg, monkeypatch, case, impl):
    run(pkg, monkeypatch, case, impl)
