"""k_pyrblur with the horizontally resized source row carried from one output row to the next (csrc/orbx_blur.hip,
pyr_finish_window: on the levels resized through the 8-byte window a row whose upper source row is the previous row's
lower one takes over its horizontal results and does not load that row).  Batches of small frames, large enough for the
two passes of the top-rows-first pipeline and too large for the short-band table (tests/pyrblur_cases.py; what the tables look
like is asserted on the host, through the library's own builders):

* pixel level: the rows of the blurred pyramid the first pass produced, read back with orbx_debug_read_pyramid_level,
  equal oracle_lib.build_level byte for byte on every level of every frame -- after the pools were filled with 0xFF and
  with 0x55 (orbx_debug_fill_pools);
* end to end: counts, keypoints, level keypoints, levels, angle bits and descriptors equal the oracle's
  detect_and_compute_gpu, with the FAST early exit (and with it the two passes) on and off.
Frames: uniform noise -- every tap and every rounding case of the resize and the blur occurs -- plus a few blocks of
0 and 255."""
import concurrent.futures as cf

import numpy as np
import pytest

import oracle_lib as O
import pyrblur_cases as PC

pytestmark = pytest.mark.gpu

PK = dict(nfeatures=500, nlevels=PC.NLEVELS, threshold=20, n=9, nms_window=3, patch_size=31, blur_levels=2, blur_kind=0)
_cache = {}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = PC.compile_mirror(tmp_path_factory.mktemp("pyrblur_bands") / "pyrblur_bands_mirror.bin", sanitize=False)
    return PC.check_shapes(exe)


def frames_of(name, n):
    case = PC.CASES[name]
    w, h = case["w"], case["h"]
    rng = np.random.default_rng(sum(map(ord, name)))
    fr = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    for f in range(n):
        for _ in range(3):  # saturated blocks, some of them across a frame border
            bw, bh = rng.integers(8, 70), rng.integers(8, 50)
            x, y = rng.integers(-8, w - 8), rng.integers(-8, h - 8)
            fr[f, max(y, 0):y + bh, max(x, 0):x + bw] = 255 * rng.integers(0, 2)
    return fr


def case_data(name, tables):
    """frames, the oracle's results and the oracle's blurred levels of a case (computed once)"""
    if name not in _cache:
        case, t = PC.CASES[name], tables[name]
        n = (-(-4096 // t["whole"]) + 7) // 8 * 8  # a wave per strip: at least 4096, or the short-band table runs
        assert n * t["whole"] >= 4096
        fr = frames_of(name, n)
        op = O.gpu_params(scale_factor=case["scale"], **PK)
        O.lib()
        with cf.ThreadPoolExecutor(16) as ex:  # ctypes releases the GIL
            refs = list(ex.map(lambda f: O.detect_and_compute_gpu(f, op), fr))
            levels = list(ex.map(lambda f: [O.build_level(f, op, l) for l in range(PC.NLEVELS)], fr))
        _cache[name] = (fr, refs, levels)
    return _cache[name]


def compare(res, refs):
    for i, ref in enumerate(refs):
        m = int(res["counts"][i])
        assert m == len(ref["kps"]), (i, m, len(ref["kps"]))
        assert np.array_equal(res["kps"][i, :m], ref["kps"]), i
        assert np.array_equal(res["kps_level"][i, :m], ref["kps_level"]), i
        assert np.array_equal(res["levels"][i, :m], ref["levels"]), i
        assert np.array_equal(res["angles"][i, :m].view(np.uint32), ref["angles"].view(np.uint32)), i
        assert np.array_equal(res["desc"][i, :m], ref["desc"]), i


def context(pkg, name, n):
    case = PC.CASES[name]
    p = pkg.default_params("gpu", max_width=case["w"], max_height=case["h"], max_batch=n, scale_factor=case["scale"], **PK)
    return pkg.Context(p)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_first_pass_rows_equal_the_oracle_pixel_for_pixel(pkg, tables, name):
    import torch

    fr, refs, levels = case_data(name, tables)
    n, (w, h) = len(fr), (PC.CASES[name]["w"], PC.CASES[name]["h"])
    d = torch.from_numpy(fr).cuda()
    torch.cuda.synchronize()
    with context(pkg, name, n) as c:
        c.set_top_rows_first(1)  # two passes whenever eligible (not the adaptive mode: the default tile rows stay)
        cap = c.plan(w, h)["out_capacity"]
        c.batch_device(d.data_ptr(), n, w, h)  # (sets the plan: the fills below reach the pyramid's pixels)
        compare(c.batch_fetch(0, n, cap), refs)
        for fill in (0xFF, 0x55):
            c.debug_fill_pools(fill)
            c.batch_device(d.data_ptr(), n, w, h)
            compare(c.batch_fetch(0, n, cap), refs)
            produced, total = c.pyramid_pixel_counts()
            assert produced < total, (produced, total)  # two passes ran, and the second one skipped strips
            for f in range(n):
                for l, (lw, lh, first, _) in enumerate(tables[name]["levels"]):
                    got = c.debug_read_pyramid_level(f, l, w, h)
                    assert got.shape == (lh, lw) == levels[f][l].shape
                    assert np.array_equal(got[:first], levels[f][l][:first]), (fill, f, l)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_batches_equal_the_oracle_with_the_early_exit_on_and_off(pkg, tables, name):
    import torch

    fr, refs, _ = case_data(name, tables)
    n, (w, h) = len(fr), (PC.CASES[name]["w"], PC.CASES[name]["h"])
    d = torch.from_numpy(fr).cuda()
    torch.cuda.synchronize()
    with context(pkg, name, n) as c:
        c.set_top_rows_first(1)
        cap = c.plan(w, h)["out_capacity"]
        for early in (True, False, True):
            c.set_fast_early_exit(early)
            c.batch_device(d.data_ptr(), n, w, h)
            compare(c.batch_fetch(0, n, cap), refs)
            produced, total = c.pyramid_pixel_counts()
            assert (produced < total) == early, (early, produced, total)  # off: one pass over the every-row table
