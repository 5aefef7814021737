"""The first pass of the FAST tile rows cut unevenly (csrc/orbx_plan.h: make_bandmap with first-pass heights; csrc/orbx_adapt.h:
adapt_tile_rows).  Tile row 0 of a level ends where most frames have filled their cap, and the units of the short
tile row 1 exit for those frames -- only the partition of the rows into units moves, so every result must stay what the
oracle computes.  ORBX_TOP_ROWS=2:r0,r1,... forces the rows of tile row 0 per level (read when a context is created); the cuts
below are worked out from the oracle's own fill rows: F = row of the cap-th survivor + 1 of a level of a frame (the
level's height if the cap never fills).  A unit of tile row 1 may leave when the rows STRICTLY above it hold the cap:
for the frames with F <= cut.

Frames: 320 x 160, 4 levels, 200 features -- seven frames of bright dots on a jittered grid, denser or sparser, whose
caps fill between rows 37 and 65 of level 0, and one frame of uniform noise with survivors in nearly every row.  Every
case runs on a pipelined context (two lanes, one graph replay per batch) with both FAST kernels, a batch of the 8 frames
and a batch of 256 (the 8 frames 32 times: large enough for the two passes of the top-rows-first pipeline), after the
working pools were filled with 0xFF -- a unit that exits leaves stale mask words behind.  A cut the kernel cannot run
(the LDS tile kernel holds 47 rows per unit) goes to the nearest one it can."""
import concurrent.futures as cf
import re

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

W, H, NL, NF, R = 320, 160, 4, 200, 1
PK = dict(nfeatures=NF, nlevels=NL, threshold=20, n=9, nms_window=3, patch_size=31, blur_levels=2, blur_kind=0)
TILE_H = 47  # orbx_fast3_tile_h(1)
REPS = 32
_cache = {}


def dots(seed, p):
    """3 x 3 bright dots, one per 10 x 10 cell with probability p, on a nearly flat background: a corner each"""
    rng = np.random.default_rng(seed)
    fr = np.full((H, W), 60, np.uint8)
    fr += rng.integers(0, 6, (H, W), dtype=np.uint8)
    for cy in range(0, H - 9, 10):
        for cx in range(0, W - 9, 10):
            if rng.random() < p:
                y, x = cy + rng.integers(3, 7), cx + rng.integers(3, 7)
                fr[y - 1:y + 2, x - 1:x + 2] = 255
    return fr


def noise(seed, amp):
    rng = np.random.default_rng(seed)
    return (128 + rng.integers(-amp, amp + 1, (H, W))).astype(np.uint8)


def level_rows():
    """per level: height, rows of a default tile row, depth of the two-row first pass"""
    out = []
    for l in range(NL):
        _, h = O.level_size(W, H, 1.2, l)
        ty = -(-h // TILE_H)
        th = -(-h // ty)
        out.append((h, th, 2 * th))
    return out


def survivors(fr, l, cap):
    op = O.gpu_params(**PK)
    return O.fast_detect(O.build_level(fr, op, l), PK["threshold"], PK["n"], PK["nms_window"], cap)


def data():
    """frames, the oracle's results, fill rows [frame][level] (computed once)"""
    if not _cache:
        fr = np.stack([dots(10 + i, p) for i, p in enumerate((1.0, 0.95, 0.9, 0.85, 0.8, 0.7, 0.6))] + [noise(3, 60)])
        op = O.gpu_params(**PK)
        O.lib()
        with cf.ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL
            refs = list(ex.map(lambda f: O.detect_and_compute_gpu(f, op), fr))
        caps = [2 * O.level_quota(NF, 1.2, NL, l) for l in range(NL)]
        fill = []
        for f in fr:
            row = []
            for l in range(NL):
                k = survivors(f, l, caps[l])
                row.append(int(k[-1][1]) + 1 if len(k) == caps[l] else level_rows()[l][0])
            fill.append(row)
        _cache["d"] = (fr, refs, np.array(fill), caps)
    return _cache["d"]


def compare(res, refs, reps=1):
    for i in range(len(refs) * reps):
        ref = refs[i % len(refs)]
        m = int(res["counts"][i])
        assert m == len(ref["kps"]), (i, m, len(ref["kps"]))
        assert np.array_equal(res["kps"][i, :m], ref["kps"]), i
        assert np.array_equal(res["kps_level"][i, :m], ref["kps_level"]), i
        assert np.array_equal(res["levels"][i, :m], ref["levels"]), i
        assert np.allclose(res["angles"][i, :m], ref["angles"], atol=1e-4, rtol=0), i
        assert np.array_equal(res["desc"][i, :m], ref["desc"]), i


def run_cut(pkg, monkeypatch, impl, cuts, big=True):
    """one context with the forced cuts: the 8 frames, the pools filled, the 8 frames on both lanes with graph replay,
    then 256 frames in two passes"""
    import torch

    fr, refs, _, _ = data()
    monkeypatch.setenv("ORBX_FAST_IMPL", impl)
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:" + ",".join(str(int(c)) for c in cuts))
    n = len(fr)
    d8 = torch.from_numpy(fr).cuda()
    d256 = torch.from_numpy(np.tile(fr, (REPS, 1, 1))).cuda() if big else None
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=n * REPS if big else n, **PK)
    with pkg.Context(p) as c:
        c.set_pipelined_batches(True)
        cap = c.plan(W, H)["out_capacity"]
        c.batch_device(d8.data_ptr(), n, W, H)  # (sets the plan: the fill below reaches the pyramid's pixels)
        compare(c.batch_fetch(0, n, cap), refs)
        c.debug_fill_pools(0xFF)
        for _ in range(4):  # both lanes, the second batch of a lane replays its graph
            c.batch_device(d8.data_ptr(), n, W, H)
            compare(c.batch_fetch(0, n, cap), refs)
        if big:
            for k in range(3):
                if k == 1:
                    c.debug_fill_pools(0xFF)
                c.batch_device(d256.data_ptr(), n * REPS, W, H)
                compare(c.batch_fetch(0, n * REPS, cap), refs, REPS)
            produced, total = c.pyramid_pixel_counts()
            assert produced < total, (produced, total)  # two passes ran, and the second one skipped strips
            worked, units = c.fast_tile_counts()
            print("cuts %s impl %s: %d of %d FAST units worked" % (list(cuts), impl, worked, units))
            assert worked < units


IMPLS = pytest.mark.parametrize("impl", ["4", "3"], ids=["fast-stream", "fast-tiles"])


def boundary_frame():
    """a (frame, level 0) whose fill row both kernels can cut at: within the LDS tile kernel's [depth - 47, 47]"""
    _, _, fill, _ = data()
    depth = level_rows()[0][2]
    ok = [f for f in range(len(fill)) if depth - TILE_H + 1 < fill[f][0] < TILE_H - 1]
    assert ok, fill[:, 0]
    return ok[0], int(fill[ok[0]][0])


@IMPLS
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_cut_at_the_fill_row_of_a_frame(pkg, monkeypatch, impl, delta):
    """rows of tile row 0 = F - 1, F, F + 1 of one frame's level 0: the frame's unit of tile row 1 may leave from F on"""
    _, F = boundary_frame()
    run_cut(pkg, monkeypatch, impl, [F + delta, 0, 0, 0])


@IMPLS
def test_every_frame_leaves_tile_row_1(pkg, monkeypatch, impl):
    """a cut below every frame's fill row, on every level that has one within its first pass"""
    _, _, fill, _ = data()
    cuts = []
    for l, (h, th, depth) in enumerate(level_rows()):
        filled = [int(v) for v in fill[:, l] if v < h]
        cuts.append(min(max(filled), depth - 1) if filled else 0)
    assert cuts[0] > 0
    run_cut(pkg, monkeypatch, impl, cuts)


@IMPLS
def test_no_frame_leaves_tile_row_1(pkg, monkeypatch, impl):
    """a cut above every frame's fill row: both tile rows of the first pass work for everybody"""
    _, _, fill, _ = data()
    run_cut(pkg, monkeypatch, impl, [max(int(fill[:, l].min()) - 1, 1) for l in range(NL)])


@pytest.mark.parametrize("rows1", [1, 6, 7, 8])
def test_short_tile_row_1(pkg, monkeypatch, rows1):
    """tile row 1 of 1, 6, 7 and 8 rows (a group of the streaming kernel has 7) on every level"""
    run_cut(pkg, monkeypatch, "4", [depth - rows1 for _, _, depth in level_rows()], big=rows1 in (1, 7))


def test_short_tile_row_1_tile_kernel(pkg, monkeypatch):
    """... the LDS tile kernel: its shortest tile row 1 leaves 47 rows to tile row 0"""
    run_cut(pkg, monkeypatch, "3", [depth - 1 for _, _, depth in level_rows()])


@pytest.mark.parametrize("rows0", [1, R + 2])
def test_short_tile_row_0(pkg, monkeypatch, rows0):
    """tile row 0 shorter than R + 3 rows: no pixel of it can hold a corner, or one row of them can"""
    run_cut(pkg, monkeypatch, "4", [rows0] * NL, big=rows0 == 1)


def test_short_tile_row_0_tile_kernel(pkg, monkeypatch):
    """... the LDS tile kernel: its shortest tile row 0 is what 47 rows of tile row 1 leave"""
    run_cut(pkg, monkeypatch, "3", [1] * NL)


@IMPLS
def test_nms_across_the_cut(pkg, monkeypatch, impl):
    """the noise frame has survivors in rows h0 - 1 and h0 of level 0, both among its first `cap`: their 3 x 3 windows
    reach across the cut"""
    fr, _, fill, caps = data()
    k = survivors(fr[-1], 0, caps[0])
    rows = np.bincount(k[:, 1], minlength=H)
    depth = level_rows()[0][2]
    ok = [h0 for h0 in range(depth - TILE_H, TILE_H + 1) if rows[h0 - 1] and rows[h0] and h0 < fill[-1][0]]
    assert ok, rows[:80]
    # the closest pair of survivors across a cut, if there is one within a window's reach
    def gap(h0):
        a, b = k[k[:, 1] == h0 - 1][:, 0], k[k[:, 1] == h0][:, 0]
        return int(np.abs(a[:, None] - b[None, :]).min())
    h0 = min(ok, key=gap)
    print("cut %d, closest survivors across it %d px apart" % (h0, gap(h0)))
    run_cut(pkg, monkeypatch, impl, [h0, 0, 0, 0])


def test_the_chooser_moves_the_cut_and_every_batch_equals_the_oracle(pkg, monkeypatch, capfd):
    """Adaptive: batches whose caps fill high up, then batches whose caps fill lower down.  The chooser cuts the first
    pass for the first content and moves the cut for the second (ORBX_TOP_ROWS=2:trace prints its decisions); every batch
    before, at and after a change equals the oracle."""
    import torch

    fr, refs, fill, _ = data()
    monkeypatch.setenv("ORBX_FAST_IMPL", "4")
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:trace")
    # content A: the four densest dot frames, content B: the three sparsest; 256 frames per batch
    sets = {"A": [0, 1, 2, 3], "B": [4, 5, 6]}
    n = 256
    idx = {k: [v[i % len(v)] for i in range(n)] for k, v in sets.items()}
    dev = {k: torch.from_numpy(fr[idx[k]]).cuda() for k in sets}
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=n, **PK)
    capfd.readouterr()
    with pkg.Context(p) as c:
        cap = c.plan(W, H)["out_capacity"]
        c.set_pipelined_batches(True)
        # (the chooser decides when an observation window ends: after 2, 6, 14 and 30 batches)
        for i in range(32):
            name = "A" if i < 6 else "B"
            c.batch_device(dev[name].data_ptr(), n, W, H)
            res = c.batch_fetch(0, n, cap)
            compare(res, [refs[j] for j in idx[name]])
    err = capfd.readouterr().err
    print(err)
    cuts = [int(m) for m in re.findall(r"level 0 need \d+ depth \d+ cut \d+ -> (\d+)", err)]
    assert err.count("re-tile") >= 2, err
    assert len({v for v in cuts if v > 0}) >= 2, (cuts, fill[:, 0])
