"""k_level_select / k_lvl_harris with the Harris window on packed 16-bit integers and the compaction walk in which
a lane owns 16 consecutive mask words (one wave scan per 1024-word chunk), bit for bit against the oracle and against
the three spread kernels (ORBX_SELECT_SPREAD=1, read once per process: a child process):

  * |gx|, |gy| at the 16-bit extreme (1020) and many tied responses, Harris windows 3, 5 and 7, 1 and 4 levels
  * candidates 3 px from every border (the window reflects one row / column), every byte alignment of a row's end
  * levels with 0, 1, 63, 64 and 65 candidates (runs of 64), caps of 1, 63, 64 and 65, and a cap reached inside a
    mask word that holds survivors on both sides of the cut
  * a cap reached past mask word 1024 of level 0 (second chunk of the walk), inside the first chunk, and never
  * a workgroup per (level, frame) (2 frames) and per frame (256 frames), also on a pipelined context

Every case states what it relies on (a gradient of 1020, a candidate on every border, the word of the cut, ...) as
an assertion on the CPU side, so a changed image or plan cannot turn it into a weaker case unnoticed.  The rows a
level needed (`need`) feed a heuristic only and are not visible through the C ABI; the flat image checks the result.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

KEYS = ("counts", "kps", "kps_level", "levels", "angles", "responses", "desc")
PLAN = ("quota", "fast_cap")

# one batch through the C ABI; argv: root, images (.npy), params (JSON), select mode, pipelined, output (.npz)
CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("visual-odometry-gpu_amd")
imgs = np.load(sys.argv[2])
kw, mode, pipelined = json.loads(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
B, h, w = imgs.shape
p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=B, select_mode=mode, **kw)
with pkg.Context(p) as c:
    plan = c.plan(w, h)
    cap = max(plan["out_capacity"], 1)
    if pipelined:  # the reversed batch on one lane, the real one on the other
        import torch
        d_rev = torch.from_numpy(np.ascontiguousarray(imgs[::-1])).cuda()
        d_img = torch.from_numpy(imgs).cuda()
        torch.cuda.synchronize()
        c.batch_host(imgs[:1])  # sets the plan: the lanes engage for an unchanged frame size
        c.set_pipelined_batches(True)
        for d in (d_rev, d_img, d_rev, d_img):
            c.batch_device(d.data_ptr(), B, w, h)
    else:
        c.batch_host(imgs)
    r = c.batch_fetch(0, B, cap)
np.savez(sys.argv[6], **{k: np.asarray(r[k]) for k in %r}, **{k: plan[k] for k in %r})
""" % (KEYS, PLAN)


def run(imgs, kw, mode, spread, tmp_path, pipelined=False):
    src, out = str(tmp_path / "imgs.npy"), str(tmp_path / ("out%d.npz" % spread))
    np.save(src, imgs)
    env = dict(os.environ, ORBX_SELECT_SPREAD=str(spread))
    subprocess.run([sys.executable, "-c", CHILD, ROOT, src, json.dumps(kw), str(mode), str(int(pipelined)), out],
                   env=env, check=True, timeout=300)
    with np.load(out) as d:
        return {k: d[k] for k in KEYS + PLAN}


def compare(imgs, kw, mode, tmp_path, oracle_frames=(0,), pipelined=False):
    """fused vs spread on every frame (Harris mode; the row-major mode has one kernel), oracle on `oracle_frames`"""
    fused = run(imgs, kw, mode, 0, tmp_path, pipelined)
    if mode == 0:
        spread = run(imgs, kw, mode, 1, tmp_path, pipelined)
        for k in KEYS:
            assert np.array_equal(fused[k].view(np.uint8), spread[k].view(np.uint8)), k
    for i in oracle_frames:
        ref = O.detect_and_compute_gpu(imgs[i], O.gpu_params(**kw)) if mode == 0 else F.rowmajor_ref(imgs[i], kw)
        n = int(fused["counts"][i])
        got = {k: fused[k][i, :n] for k in KEYS if k != "counts"}
        got["count"] = n
        F.check(got, ref, (i, kw, mode))
    return fused


BASE = dict(nfeatures=500, nlevels=1, scale_factor=1.2, threshold=20, n=9, nms_window=3, patch_size=31,
            harris_window=7, harris_k=0.04, blur_levels=0, blur_kind=0)


def noise(seed, h, w):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(100.0 + 40.0 * rng.standard_normal((h, w))), 0, 255).astype(np.uint8)


def blocks(seed, h, w, cell=3, period=24):
    """cells of 0 / 255, the same 24 x 24 pattern over the frame, plus one bit of noise at 2 % of the pixels: Sobel sums
    reach +-1020, and the repeated neighbourhoods give many candidates the same response"""
    rng = np.random.default_rng(seed)
    tile = np.kron(rng.integers(0, 2, (period // cell, period // cell)), np.ones((cell, cell), np.int64))
    img = np.tile(tile, ((h + period - 1) // period, (w + period - 1) // period))[:h, :w] * 255
    return np.clip(img + (rng.random((h, w)) < 0.02), 0, 255).astype(np.uint8)


def survivors(img, kw):
    """level 0's FAST + NMS survivors in the order of the compaction walk (row-major), all of them"""
    return O.fast_detect(img, kw["threshold"], kw["n"], kw["nms_window"], img.size)


def mask_word(x, y, w):
    """index of the level-0 mask word of pixel (x, y): strips of 248 px (62 dwords), four 64-bit words per strip"""
    strip_px = 248
    strips = max(1, ((w + 3) // 4 - 2 + 61) // 62)
    return y * 4 * strips + (x // strip_px) * 4 + (x % strip_px) // 64


def level_counts(r, i, nlevels):
    return np.bincount(r["levels"][i, :int(r["counts"][i])], minlength=nlevels)


# ---- 16-bit extremes and ties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlevels", [1, 4])
@pytest.mark.parametrize("harris_window", [3, 5, 7])
def test_extremes_and_ties(tmp_path, harris_window, nlevels):
    imgs = np.stack([blocks(10 * harris_window + nlevels + k, 64, 96) for k in range(2)])
    for img in imgs:  # the Sobel sums of the interior reach both 16-bit extremes
        p = img.astype(np.int64)
        gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
        gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
        assert gx.max() == 1020 and gx.min() == -1020 and gy.max() == 1020 and gy.min() == -1020
    kw = dict(BASE, nfeatures=60 * nlevels, nlevels=nlevels, harris_window=harris_window)
    r = compare(imgs, kw, 0, tmp_path, oracle_frames=(0, 1))
    resp = r["responses"][0, :int(r["counts"][0])]
    assert len(resp) - len(np.unique(resp)) >= 10, "too few tied responses among the selected keypoints"


# ---- borders ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 65, 66, 67])
def test_borders(tmp_path, width):
    h = 48
    imgs = np.stack([noise(7 * width + k, h, width) for k in range(2)])
    kw = dict(BASE, nfeatures=256)  # cap 512: above the number of survivors, every one of them is a candidate
    r = compare(imgs, kw, 0, tmp_path, oracle_frames=(0, 1))
    assert all(len(survivors(img, kw)) < 256 for img in imgs), "the quota cuts candidates off"
    kps = np.concatenate([r["kps"][i, :int(r["counts"][i])] for i in range(2)])
    x, y = kps[:, 0], kps[:, 1]
    # the 9 x 9 neighbourhood of a candidate 3 px from a border reflects one column / row
    assert (x == 3).any() and (x == width - 4).any() and (y == 3).any() and (y == h - 4).any()


# ---- run and cap boundaries ---------------------------------------------------------------------------------------
def dots(n):
    """n isolated bright pixels, each exactly one FAST survivor, with different contrasts"""
    img = np.full((96, 128), 90, np.uint8)
    for c in range(n):
        img[8 + 12 * (c // 10), 6 + 12 * (c % 10)] = 250 - 9 * (c % 7)
    return img


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_candidates_per_level(tmp_path, n):
    imgs = np.stack([dots(n), dots(max(n - 1, 0))])
    kw = dict(BASE, nfeatures=100)
    assert len(survivors(imgs[0], kw)) == n
    r = compare(imgs, kw, 0, tmp_path, oracle_frames=(0, 1))
    assert int(r["counts"][0]) == n


@pytest.mark.parametrize("mode,nfeatures", [(1, 1), (1, 63), (1, 64), (1, 65), (0, 32)])
def test_caps(tmp_path, mode, nfeatures):
    # the walk stops at the cap: 1, 63, 64 and 65 survivors in row-major mode (cap = nfeatures), one run of exactly
    # 64 candidates in Harris mode (cap = 2 * quota)
    imgs = np.stack([noise(nfeatures + k, 64, 96) for k in range(2)])
    kw = dict(BASE, nfeatures=nfeatures)
    r = compare(imgs, kw, mode, tmp_path, oracle_frames=(0, 1))
    assert int(r["fast_cap"][0]) == (nfeatures if mode else 64)
    assert int(r["counts"][0]) == nfeatures


def test_cap_inside_a_mask_word(tmp_path):
    img = noise(77, 64, 96)
    kw = dict(BASE, nfeatures=45)  # cap 90
    s = survivors(img, kw)
    words = [mask_word(int(x), int(y), 96) for x, y in s]
    # survivors 88, 89 (kept) and 90 (cut off) share a mask word
    assert len(s) > 91 and words[88] == words[89] == words[90], words[86:93]
    r = compare(np.stack([img, img[::-1].copy()]), kw, 0, tmp_path, oracle_frames=(0, 1))
    assert int(r["fast_cap"][0]) == 90


# ---- chunk boundary -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["late", "early", "flat"])
def test_chunks(tmp_path, kind):
    h, w = 200, 640
    img = noise(5, h, w)
    if kind == "late":
        img[:90] = 100
    elif kind == "flat":
        img[:] = 100
    kw = dict(BASE, nfeatures=400, nlevels=2)
    r0 = None
    if kind != "flat":
        s = survivors(img, kw)
        cap = 2 * O.level_quota(400, 1.2, 2, 0)
        assert len(s) > cap
        word = mask_word(int(s[cap - 1][0]), int(s[cap - 1][1]), w)
        first = mask_word(int(s[0][0]), int(s[0][1]), w)
        # a chunk of the walk is 1024 words: the cut lies in the second chunk and nothing in the first / in the first
        assert (first >= 1024 and 1024 <= word < 2048) if kind == "late" else word < 1024, (first, word)
        r0 = cap
    r = compare(np.stack([img, img[:, ::-1].copy()]), kw, 0, tmp_path, oracle_frames=(0, 1))
    if kind == "flat":
        assert int(r["counts"].max()) == 0
    else:
        assert int(r["fast_cap"][0]) == r0 and level_counts(r, 0, 2)[0] == r["quota"][0]


# ---- both workgroup shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("frames", [2, 256])
def test_workgroup_shapes(tmp_path, frames, pipelined):
    two = np.stack([blocks(3, 64, 96), noise(4, 64, 96)])
    imgs = two[np.arange(frames) % 2]
    kw = dict(BASE, nfeatures=240, nlevels=4)
    compare(imgs, kw, 0, tmp_path, oracle_frames=(0, frames - 1), pipelined=pipelined)
