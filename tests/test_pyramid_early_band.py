"""The early band of the fused pyramid + blur kernel's second pass (csrc/orbx_plan.h: pyrblur_early_rows,
build_pyrblur_tiles with early_rows; csrc/orbx_adapt.h: choose_early_bands).  With the first pass of the FAST tile rows cut at h0
(tile row 0) and D (end of tile row 1), the pyramid rows [P, D + 21) with P = max(h0 + 21, D + R + 3) leave the first
pyramid launch and become second-pass strips that are skipped for the frames whose cap filled within tile row 0.  Only
where rows are produced moves, so every result must stay what the oracle computes; a row that was wrongly left out
shows as a wrong descriptor, because the pools are filled with 0xFF and 0x55 before the batches.

Set-up as in tests/test_fast_first_split.py: frames 320 x 160, 4 levels, 200 features, the cuts forced through
ORBX_TOP_ROWS=2:r0,... (under a forced cut the band is applied wherever it has three rows or more), pipelined lanes
with graph replay, both FAST kernels.  Level 0 has 160 rows, a first pass of D = 80 rows and cap 128: with a cut h0 the
band is rows [max(h0 + 21, 84), 101): up to h0 = 63 the first launch ends where its FAST units stop reading (row 84),
from h0 = 64 on where the descriptors of tile row 0's keypoints do (h0 + 21).  The LDS tile kernel holds 47 rows per
unit, so it moves a forced cut into [33, 47] and only the streaming kernel reaches the second regime at this frame
size.  The two-pass run takes 256 frames, the smallest batch that runs in two passes
(the strip table of this size has 16 strips, and below 4096 waves a batch takes the short-band table in one pass --
checked below with a batch of 248).

Frames (fill row F of level 0 = row of the cap-th survivor + 1, checked on the CPU with the oracle in
test_frames_have_their_fill_rows):
  0 .. 3  dots frames of tests/test_fast_first_split.py, F = 37, 45, 47, 65
  4       its noise frame, F = 65, levels 1 .. 3 never fill
  5       built: the cap-th survivor in row 79, the last row of tile row 1 (F = D = 80): its descriptor reaches row 99
  6       built: the cap-th survivor in row 40 (F = 41): with the cut at 41 it fills in row h0 - 1 and its band is
          skipped; its descriptors reach row 60, far above the first launch's end at row 84 (a cut both kernels can run)
  7       sparse dots: no level ever fills
  8       built: the cap-th survivor in row 69 (F = 70): with the cut at 70 the first launch ends at P = h0 + 21 = 91
          (> D + R + 3 = 84), the band is rows [91, 101) and is skipped for this frame, and the descriptors of its
          row-69 keypoints read up to row 89, the first launch's last row but one (the margin has one spare row).  Not
          among the eight frames of the other cases (ALL).
"""
import concurrent.futures as cf

import numpy as np
import pytest

import oracle_lib as O
import test_fast_first_split as S

W, H, NL, R = S.W, S.H, S.NL, S.R
MARGIN = 21  # ORBX_TOP_MARGIN
_cache = {}


def caps():
    return [2 * O.level_quota(S.NF, 1.2, NL, l) for l in range(NL)]


def built(target, seed):
    """3 x 3 bright dots 8 px apart: cap - 1 of them well above row target - 1, then a row of them centred in it"""
    rng = np.random.default_rng(seed)
    fr = np.full((H, W), 60, np.uint8)
    fr += rng.integers(0, 6, (H, W), dtype=np.uint8)
    pts = [(x, y) for y in range(5, target - 1 - 7, 8) for x in range(5, W - 5, 8)][:caps()[0] - 1]
    pts += [(x, target - 1) for x in range(5, W - 5, 8)]
    pts += [(x, y) for y in range(target + 8, H - 5, 10) for x in range(5, W - 5, 10)]
    for x, y in pts:
        fr[y - 1:y + 2, x - 1:x + 2] = 255
    return fr


def data():
    """frames, the oracle's results, fill rows [frame][level] (computed once)"""
    if not _cache:
        fr = np.stack([S.dots(10 + i, p) for i, p in ((0, 1.0), (2, 0.9), (4, 0.8), (6, 0.6))] +
                      [S.noise(3, 60), built(80, 5), built(41, 6), S.dots(99, 0.08), built(70, 8)])
        op = O.gpu_params(**S.PK)
        O.lib()
        with cf.ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL
            refs = list(ex.map(lambda f: O.detect_and_compute_gpu(f, op), fr))
        fill = []
        for f in fr:
            row = []
            for l in range(NL):
                k = S.survivors(f, l, caps()[l])
                row.append(int(k[-1][1]) + 1 if len(k) == caps()[l] else S.level_rows()[l][0])
            fill.append(row)
        _cache["d"] = (fr, refs, np.array(fill))
    return _cache["d"]


def band_rows(h0, l=0):
    """rows [P, S) of the level's early band under the cut h0"""
    h, _, depth = S.level_rows()[l]
    return min(h, max(h0 + MARGIN, depth + R + 3)), min(h, depth + MARGIN)


def test_frames_have_their_fill_rows(oracle):
    _, refs, fill = data()
    h, _, depth = S.level_rows()[0]
    assert (h, depth, caps()[0]) == (160, 80, 128)
    assert list(fill[:, 0]) == [37, 45, 47, 65, 65, depth, 41, h, 70], fill
    assert list(fill[7]) == [lr[0] for lr in S.level_rows()]  # the sparse frame never fills
    # frame 5: level-0 keypoints in row 79, the last of tile row 1; frame 6: in row 40 and none below
    for i, row in ((5, depth - 1), (6, 40), (8, 69)):
        y = refs[i]["kps_level"][refs[i]["levels"] == 0][:, 1]
        assert int(y.max()) == row, (i, int(y.max()))
    # the band the cuts below leave has rows, and ends where the first pass ended before
    for h0 in (36, 37, 38, 41, 47, 65):
        p, s = band_rows(h0)
        assert s == 101 and p == max(h0 + 21, 84) and s - p >= 3
    # ... and in all of them the first launch ends where its FAST units stop reading; under the cut at frame 8's fill
    # row it ends where the descriptors of tile row 0's keypoints do, one row below the last one frame 8 reads
    assert all(band_rows(h0)[0] == depth + R + 3 for h0 in (36, 37, 38, 41, 47))
    p, s = band_rows(70)
    assert p == 70 + MARGIN == 91 and p > depth + R + 3 and s - p == 10
    assert 69 + 20 == p - 2  # (DESC_R = 20 rows below the keypoint)


def run_cut(pkg, monkeypatch, impl, cuts, frames, late=False, fills=(0xFF, 0x55)):
    """one context with the forced cuts on the chosen frames: a small batch, the pools filled, small batches on both
    lanes with graph replay, then batches of >= 256 frames in two passes.  Returns the pixels produced and their total."""
    import torch

    fr, refs, _ = data()
    fr, refs = fr[list(frames)], [refs[i] for i in frames]
    n = len(fr)
    reps = -(-256 // n)
    monkeypatch.setenv("ORBX_FAST_IMPL", impl)
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:" + ("late:" if late else "") + ",".join(str(int(c)) for c in cuts))
    dn = torch.from_numpy(fr).cuda()
    dbig = torch.from_numpy(np.tile(fr, (reps, 1, 1))).cuda()
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=n * reps, **S.PK)
    with pkg.Context(p) as c:
        c.set_pipelined_batches(True)
        cap = c.plan(W, H)["out_capacity"]
        c.batch_device(dn.data_ptr(), n, W, H)  # (sets the plan: the fills below reach the pyramid's pixels)
        S.compare(c.batch_fetch(0, n, cap), refs)
        for fill in fills:
            c.debug_fill_pools(fill)
            for _ in range(2):  # both lanes
                c.batch_device(dn.data_ptr(), n, W, H)
                S.compare(c.batch_fetch(0, n, cap), refs)
            for k in range(2):  # both lanes; the second batch of a lane replays its graph
                c.batch_device(dbig.data_ptr(), n * reps, W, H)
                S.compare(c.batch_fetch(0, n * reps, cap), refs, reps)
            c.debug_fill_pools(fill)
            c.batch_device(dbig.data_ptr(), n * reps, W, H)
            S.compare(c.batch_fetch(0, n * reps, cap), refs, reps)
        return c.pyramid_pixel_counts()


IMPLS = pytest.mark.parametrize("impl", ["4", "3"], ids=["fast-stream", "fast-tiles"])
ALL = tuple(range(8))


def expected_pixels(frames, cuts, late):
    """what the second pass leaves out, from the oracle's fill rows: per (frame, level with a second pass) the rows
    below the first pass where the cap fills within it, and the band's rows where it fills within tile row 0.  (Holds
    while the tile rows keep their default heights: with all eight frames, two of which never fill.)"""
    _, _, fill = data()
    reps = -(-256 // len(frames))
    done = total = 0
    for f in frames:
        for l, (h, th, depth) in enumerate(S.level_rows()):
            w, _ = O.level_size(W, H, 1.2, l)
            total += w * h
            s = min(h, depth + MARGIN)
            rows = h
            if h > depth and s < h and fill[f][l] <= depth:  # (a level of two tile rows has no second pass)
                rows = s
                if not late and cuts[l] > 0 and fill[f][l] <= cuts[l]:
                    p, _ = band_rows(cuts[l], l)
                    if s - p >= 3:
                        rows = p
            done += w * rows
    return done * reps, total * reps


@pytest.mark.gpu
def test_the_band_is_skipped_and_counted(pkg, monkeypatch):
    """cuts at 47, 40 and 33 rows of levels 0 .. 2 (forced on every level with a second pass, so that the chooser
    moves nothing meanwhile; with all eight frames the tile rows keep their default heights, two frames never fill):
    the frames that fill within tile row 0 leave their band out, exactly the pixels the oracle's fill rows say; with
    ORBX_TOP_ROWS=2:late nothing of the first pass is left out; and a batch of 248 frames runs in one pass"""
    cuts = [47, 40, 33, 0]
    produced, total = run_cut(pkg, monkeypatch, "4", cuts, ALL)
    late, total_late = run_cut(pkg, monkeypatch, "4", cuts, ALL, late=True, fills=(0xFF,))
    assert total == total_late and produced < late < total, (produced, late, total)
    assert (produced, total) == expected_pixels(ALL, cuts, False), (produced, total, expected_pixels(ALL, cuts, False))
    assert (late, total) == expected_pixels(ALL, cuts, True), (late, total, expected_pixels(ALL, cuts, True))

    import torch

    fr, refs, _ = data()
    fr, refs = fr[:8], refs[:8]
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:47,40,33,0")
    d = torch.from_numpy(np.tile(fr, (31, 1, 1))).cuda()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=248, **S.PK)
    with pkg.Context(p) as c:
        cap = c.plan(W, H)["out_capacity"]
        c.batch_device(d.data_ptr(), 248, W, H)
        S.compare(c.batch_fetch(0, 248, cap), refs, 31)
        one_pass, t = c.pyramid_pixel_counts()
        assert one_pass == t


@pytest.mark.gpu
@IMPLS
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_cut_at_the_fill_row_of_a_frame(pkg, monkeypatch, impl, delta):
    """rows of tile row 0 = F - 1, F, F + 1 of frame 0's level 0 (F = 37): its band is skipped from F on"""
    _, _, fill = data()
    F = int(fill[0][0])
    produced, total = run_cut(pkg, monkeypatch, impl, [F + delta, 0, 0, 0], ALL, fills=(0xFF,))
    assert produced < total


@pytest.mark.gpu
@IMPLS
def test_cap_fills_in_the_last_row_of_tile_row_1(pkg, monkeypatch, impl):
    """frame 5 alone and among the others: its descriptors read the band's rows up to row 99"""
    for frames in ((5,), ALL):
        produced, total = run_cut(pkg, monkeypatch, impl, [41, 0, 0, 0], frames, fills=(0x55,))
        assert produced < total


@pytest.mark.gpu
@IMPLS
def test_cap_fills_in_the_last_row_of_tile_row_0(pkg, monkeypatch, impl):
    """frame 6 with the cut at its fill row 41, which both kernels can run: it fills in row h0 - 1 and its band is
    skipped (the first launch ends at row 84 here, far below what its descriptors read)"""
    produced, total = run_cut(pkg, monkeypatch, impl, [41, 0, 0, 0], (6,))
    assert produced < total


@pytest.mark.gpu
@IMPLS
def test_descriptors_read_the_first_launch_s_last_rows(pkg, monkeypatch, impl):
    """frame 8 with the cut at its fill row 70, alone and with the other eight: the first launch ends at h0 + 21 = 91,
    the frame's band [91, 101) is skipped, and the descriptors of its keypoints in row h0 - 1 = 69 read rows up to 89 --
    a first launch that ended a few rows earlier would hand them the fill byte.  (The LDS tile kernel moves the cut to
    47: it runs the same frames with the first launch ending at row 84.)"""
    cuts = [70, 40, 33, 0]
    for frames in ((8,), ALL + (8,)):
        produced, total = run_cut(pkg, monkeypatch, impl, cuts, frames)
        assert produced < total
    if impl == "4":  # (nine frames, two of which never fill: default tile-row heights, so the count is exact)
        frames = ALL + (8,)
        assert (produced, total) == expected_pixels(frames, cuts, False), (produced, total)
        assert produced < expected_pixels(frames, cuts, True)[0]


@pytest.mark.gpu
@IMPLS
def test_every_frame_leaves(pkg, monkeypatch, impl):
    """frames 0 .. 2 and 6 under a cut below all their fill rows, on every level that has one within its first pass"""
    _, _, fill = data()
    frames = (0, 1, 2, 6)
    cuts = []
    for l, (h, th, depth) in enumerate(S.level_rows()):
        filled = [int(fill[f][l]) for f in frames if fill[f][l] < h]
        cuts.append(min(max(filled), depth - 1) if filled else 0)
    assert cuts[0] == 47
    produced, total = run_cut(pkg, monkeypatch, impl, cuts, frames)
    assert produced < total


@pytest.mark.gpu
@IMPLS
def test_no_frame_leaves(pkg, monkeypatch, impl):
    """a cut above every frame's fill row: the band is produced for everybody, the rest still skipped"""
    _, _, fill = data()
    cuts = [max(int(fill[:, l].min()) - 1, 1) for l in range(NL)]
    produced, total = run_cut(pkg, monkeypatch, impl, cuts, ALL, fills=(0xFF,))
    if impl == "4":  # (the LDS tile kernel moves a cut it cannot run: the counts then follow other cuts)
        assert (produced, total) == expected_pixels(ALL, cuts, False) and produced < total


@pytest.mark.gpu
@IMPLS
def test_a_frame_that_never_fills(pkg, monkeypatch, impl):
    """frame 7 alone: every strip of the second pass is produced"""
    produced, total = run_cut(pkg, monkeypatch, impl, [47, 45, 37, 0], (7,), fills=(0x55,))
    assert produced == total


@pytest.mark.gpu
def test_two_frame_sizes_alternating(pkg, monkeypatch):
    """320 x 160 and its 288 x 144 corner in turn on one context: the tables, bands included, are rebuilt at every change"""
    import torch

    fr, refs, _ = data()
    fr, refs = fr[:8], refs[:8]
    w2, h2 = 288, 144
    small = np.ascontiguousarray(fr[:, :h2, :w2])
    op = O.gpu_params(**S.PK)
    with cf.ThreadPoolExecutor(8) as ex:
        refs2 = list(ex.map(lambda f: O.detect_and_compute_gpu(f, op), small))
    monkeypatch.setenv("ORBX_FAST_IMPL", "4")
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:41,40,33,0")
    reps = 40  # (the smaller size has 13 strips per frame: two passes from 316 frames on)
    big = {(W, H): (torch.from_numpy(np.tile(fr, (reps, 1, 1))).cuda(), refs),
           (w2, h2): (torch.from_numpy(np.tile(small, (reps, 1, 1))).cuda(), refs2)}
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=8 * reps, **S.PK)
    with pkg.Context(p) as c:
        c.set_pipelined_batches(True)
        for i, size in enumerate([(W, H), (w2, h2)] * 3):
            d, rf = big[size]
            cap = c.plan(*size)["out_capacity"]
            if i in (2, 3):
                c.debug_fill_pools(0xFF if i == 2 else 0x55)
            for _ in range(2):
                c.batch_device(d.data_ptr(), 8 * reps, *size)
                S.compare(c.batch_fetch(0, 8 * reps, cap), rf, reps)
            produced, total = c.pyramid_pixel_counts()
            assert produced < total, (size, produced, total)


@pytest.mark.gpu
def test_the_rule_splits_on_its_own(pkg, monkeypatch, capfd):
    """Adaptive, nothing forced: frames 0 .. 2 and 6 (caps full after 37 .. 47 rows of level 0).  The chooser cuts the
    first pass at the end of an observation window, set_plan asks early_band_pays with that window's histograms
    (ORBX_TOP_ROWS=2:trace prints its answers), and every batch before, at and after the change equals the oracle."""
    import torch

    fr, refs, _ = data()
    idx = [(0, 1, 2, 6)[i % 4] for i in range(256)]
    monkeypatch.setenv("ORBX_FAST_IMPL", "4")
    monkeypatch.setenv("ORBX_TOP_ROWS", "2:trace")
    d = torch.from_numpy(fr[idx]).cuda()
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=256, **S.PK)
    capfd.readouterr()
    with pkg.Context(p) as c:
        cap = c.plan(W, H)["out_capacity"]
        c.set_pipelined_batches(True)
        for i in range(16):  # (observation windows end after 2, 6 and 14 batches)
            if i in (7, 15):
                c.debug_fill_pools(0xFF if i == 7 else 0x55)
            c.batch_device(d.data_ptr(), 256, W, H)
            S.compare(c.batch_fetch(0, 256, cap), [refs[j] for j in idx])
        produced, total = c.pyramid_pixel_counts()
    err = capfd.readouterr().err
    print(err)
    bands = [ln for ln in err.splitlines() if ln.startswith("orbx early band")]
    assert any(ln.endswith(": split") for ln in bands), err
    assert not any("forced" in ln for ln in bands)
    assert produced < total
