"""The batched path on the inputs a drop-in caller really hands over: regions of a larger image (any row stride, any
base alignment), frames with gaps between them, frames smaller than the context's maximum, and sizes that change
during the life of a context.

Everything is compared BIT FOR BIT with the CPU oracle run on a contiguous copy of the same pixels: counts,
keypoints, level keypoints, levels and descriptors equal, angles and responses equal as float bit patterns.

1. strided / unaligned input (`CASES` x `VARIANTS`): every case runs six times on the same pointer -- surroundings
   0x00, surroundings 0xFF (the bytes between rows and frames must not matter), new pixels (a replayed graph must
   read the current memory) --, plus two stride pairs alternating on one pointer, the host entry and the argument
   errors;
2. frames smaller than the maximum and size changes within one context, dense content before a change and sparse
   content after it, plain / pipelined / host-written results, across an adaptive re-tile, and with the working pools
   filled with 0xFF / 0x55 (orbx_debug_fill_pools) before every batch;
3. the 600 x 1100 context with 594 x 1084 frames whose caps fill in the top rows (first finding; the host
   sweep of tests/test_plan_capacity.py is the check of the arithmetic, this is the end-to-end confirmation).
"""
import numpy as np
import pytest

from test_gpu_parity import synth
from test_headline_parity import PK, oracle_on

pytestmark = pytest.mark.gpu

W, H = 1241, 376
COMPARISONS = [0]  # (case, frame) comparisons made so far (reported by test_zz_report)


def check(res, refs, nlevels=None, compact=False):
    """res: what a fetch or a host view delivers for the frames of `refs`; bit for bit."""
    # (copies: a view of the pinned mirror dangles once the context is closed)
    res = {k: (None if v is None or isinstance(v, int) else np.array(v)) for k, v in res.items()}
    for i, ref in enumerate(refs):
        n = int(res["counts"][i])
        assert n == len(ref["kps"]), (i, n, len(ref["kps"]))
        assert res.get("kps") is not None or res.get("kps16") is not None
        if res.get("kps") is not None:
            assert np.array_equal(res["kps"][i, :n], ref["kps"]), i
        if res.get("kps16") is not None:
            assert np.array_equal(res["kps16"][i, :n].astype(np.int32), ref["kps"]), i
        assert np.array_equal(res["angles"][i, :n].view(np.uint32), ref["angles"].view(np.uint32)), i
        assert np.array_equal(res["desc"][i, :n], ref["desc"]), i
        if not compact:
            assert np.array_equal(res["kps_level"][i, :n], ref["kps_level"]), i
            assert np.array_equal(res["levels"][i, :n], ref["levels"]), i
            assert np.array_equal(res["responses"][i, :n].view(np.uint32), ref["responses"].view(np.uint32)), i
        if nlevels is not None:  # a case must not pass empty: every pyramid level delivered keypoints
            assert np.array_equal(np.unique(ref["levels"]), np.arange(nlevels)), (i, np.unique(ref["levels"]))
        COMPARISONS[0] += 1


# ---------------------------------------------------------------------------
# 1. strided and unaligned input

# source-read modes of k_pyrblur / k_pyramid2: level 0 always; scale <= 2 per level: the 8-byte window; 2..3.2: the
# staged rows (or, single-strip levels and widths that do not satisfy the staging rule, the 2-byte gathers); the 8
# levels of s12 reach scale 3.6 and so pass through window, staged and gather levels.  Staged cases as in
# test_staged_resize_levels: caps above the number of corners of the staged level, so that every pixel of it matters.
KW = {
    "s12": dict(nfeatures=3000, nlevels=8, scale_factor=1.2, threshold=20),
    "s15": dict(nfeatures=3000, nlevels=5, scale_factor=1.5, threshold=20),
    "s20": dict(nfeatures=3000, nlevels=4, scale_factor=2.0, threshold=20),
    "s21": dict(nfeatures=2800, nlevels=3, scale_factor=2.1, threshold=25),
    "s26": dict(nfeatures=2800, nlevels=3, scale_factor=2.6, threshold=25),
    "s31": dict(nfeatures=2800, nlevels=3, scale_factor=3.1, threshold=25),
    "kitti": {k: v for k, v in PK.items() if k not in ("blur_levels", "blur_kind")},
}
VARIANTS = {  # name: (blur_levels, fused pyramid + blur)
    "fused": (2, True),      # k_pyrblur reads the caller's frame
    "unfused": (2, False),   # k_pyramid2 does, the blur runs on the pool
    "noblur": (0, True),     # k_pyramid2, no blur at all
}


def region(name, kw, w, h, n, x0, y0, wp, hp, top=2):
    """n frames as regions at (y0, x0) of a parent of shape (n, hp, wp)"""
    assert x0 + w <= wp and y0 + h <= hp
    return dict(name=name, kw=kw, w=w, h=h, n=n, base=y0 * wp + x0, rs=wp, fs=hp * wp, top=top)


def raw(name, kw, w, h, n, base, rs, fs):
    return dict(name=name, kw=kw, w=w, h=h, n=n, base=base, rs=rs, fs=fs, top=2)


def make_cases():
    c = []
    # base misalignment 0..7 with an aligned parent width; parent widths of every residue mod 4 (the row starts walk
    # through all alignments); both at once
    for x0 in range(8):
        c.append(region("x0=%d,wp=656" % x0, "s12", 643, 200, 3, x0, 2, 656, 205))
    for wp in (652, 653, 654, 655):
        c.append(region("x0=0,wp=%d" % wp, "s12", 643, 200, 3, 0, 1, wp, 203))
    for x0, wp in ((3, 653), (5, 654), (6, 655), (1, 657)):
        c.append(region("x0=%d,wp=%d" % (x0, wp), "s12", 643, 200, 3, x0, 2, wp, 204))
    # tight rows with a gap between the frames that is no multiple of 4; padded rows with the frames back to back
    # (frame_stride = row_stride * (height - 1) + width, the smallest the entry accepts)
    c.append(raw("rows-tight,gap=3", "s12", 643, 200, 3, 0, 643, 643 * 200 + 3))
    c.append(raw("rows-tight,gap=5,base=1", "s15", 643, 200, 3, 1, 643, 643 * 200 + 5))
    c.append(raw("rows-padded,back-to-back", "s12", 643, 200, 3, 0, 650, 650 * 199 + 643))
    c.append(raw("rows-padded-odd,back-to-back,base=3", "s26", 643, 200, 3, 3, 649, 649 * 199 + 643))
    # widths of every residue mod 4 (one and several strips per level; 250: the single-strip level that falls back to
    # the 2-byte gathers) x every source-read mode, heights around 200
    for k, (w, h) in enumerate(((1241, 200), (1022, 199), (643, 201), (600, 203), (250, 200))):
        for j, kw in enumerate(("s12", "s15", "s20", "s21", "s26", "s31")):
            x0 = (3 * k + 5 * j + 1) % 8
            wp = w + 8 + (k + j) % 4
            c.append(region("w=%d,%s,x0=%d,wp=%d" % (w, kw, x0, wp), kw, w, h, 3, x0, 1, wp, h + 3))
    # batch sizes 1 and > 32
    c.append(region("n=1,x0=3,wp=653", "s12", 643, 200, 1, 3, 2, 653, 205))
    c.append(region("n=1,w=1241,s26", "s26", 1241, 200, 1, 5, 0, 1251, 200))
    c.append(region("n=33,x0=5,wp=654", "s12", 643, 200, 33, 5, 1, 654, 202))
    # the KITTI shape, 40 frames (a batch large enough for the two passes of the top-rows-first pipeline, whose
    # first-pass and rest tables both read the source): adaptive, always, never
    for top in (2, 1, 0):
        c.append(region("kitti,n=40,top=%d" % top, "kitti", W, H, 40, 3, 2, 1251, 380, top=top))
    return c


CASES = make_cases()
CASE_PARAMS = [pytest.param(c, v, id="%s-%s" % (v, c["name"])) for v in VARIANTS for c in CASES
               if c["top"] == 2 or v == "fused"]  # (the top-rows-first pipeline exists in the fused kernel only)


def case_frames(case, gen):
    """keypoint-rich frames of a case: noise and rectangles in turn; gen 0 / 1: the pixels before / after the change"""
    # (the three KITTI cases differ in the mode only: same frames, one oracle run)
    seed = (sum(map(ord, case["name"].split(",top=")[0])) * 7 + 1000 * gen) % 100000
    return np.stack([synth(seed + i, case["h"], case["w"], "rects" if (i + gen) % 2 else "noise")
                     for i in range(case["n"])])


_oracle_cache = {}


def case_oracle(case, blur_levels, gen):
    key = (case["name"].split(",top=")[0], blur_levels, gen)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle_on(case_frames(case, gen), dict(KW[case["kw"]], blur_levels=blur_levels))
    return _oracle_cache[key]


def pack(case, frames, fill, tail=3):
    """the parent buffer: every byte `fill` except the regions, which hold the frames"""
    n, h, w = frames.shape
    size = case["base"] + (n - 1) * case["fs"] + (h - 1) * case["rs"] + w + tail
    buf = np.full(size, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[case["base"]:], shape=(n, h, w), strides=(case["fs"], case["rs"], 1))
    view[...] = frames
    # the oracle's input: a contiguous copy of exactly what the regions hold
    assert np.array_equal(np.ascontiguousarray(view), frames)
    return buf


@pytest.mark.parametrize("case,variant", CASE_PARAMS)
def test_strided_regions(pkg, case, variant):
    import torch

    blur_levels, fused = VARIANTS[variant]
    kw = dict(KW[case["kw"]], blur_levels=blur_levels)
    w, h, n = case["w"], case["h"], case["n"]
    frames = [case_frames(case, g) for g in (0, 1)]
    refs = [case_oracle(case, blur_levels, g) for g in (0, 1)]
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=n, **kw)
    with pkg.Context(p) as c:
        c.set_fused_pyramid_blur(fused)
        c.set_top_rows_first(case["top"])
        cap = c.plan(w, h)["out_capacity"]
        t = torch.from_numpy(pack(case, frames[0], 0x00)).cuda()
        torch.cuda.synchronize()
        ptr = t.data_ptr() + case["base"]

        def run():
            c.batch_device(ptr, n, w, h, row_stride=case["rs"], frame_stride=case["fs"])
            return c.batch_fetch(0, n, cap)

        # (a captured launch sequence belongs to one of the FOUR result blocks the batches take in turn: calls 1-4
        # capture, from the fifth call on the sequences are replayed)
        check(run(), refs[0], kw["nlevels"])          # surroundings 0x00
        t.copy_(torch.from_numpy(pack(case, frames[0], 0xFF)))
        torch.cuda.synchronize()
        check(run(), refs[0], kw["nlevels"])          # surroundings 0xFF, same pointer
        for _ in range(2):
            c.batch_device(ptr, n, w, h, row_stride=case["rs"], frame_stride=case["fs"])
        c.wait()
        t.copy_(torch.from_numpy(pack(case, frames[1], 0xFF)))
        torch.cuda.synchronize()
        check(run(), refs[1], kw["nlevels"])          # new pixels in the regions: the replay of call 1 reads them
        check(run(), refs[1], kw["nlevels"])          # ... and the replay of call 2


def test_two_stride_pairs_alternate_on_one_pointer(pkg):
    """The captured launch sequences are keyed by pointer AND strides: one buffer read as 3 frames of 643 x 200 with
    (row_stride, frame_stride) = (650, 650 * 205) and with (655, 655 * 203 + 1) in turn; then the pixels change
    and both are read again."""
    import torch

    w, h, n = 643, 200, 3
    kw = dict(KW["s12"], blur_levels=2)
    pairs = [(650, 650 * 205), (655, 655 * 203 + 1)]
    size = 2 + max((n - 1) * fs + (h - 1) * rs + w for rs, fs in pairs)

    def views(buf):
        return [np.ascontiguousarray(np.lib.stride_tricks.as_strided(buf[2:], shape=(n, h, w), strides=(fs, rs, 1)))
                for rs, fs in pairs]

    bufs = [synth(77 + g, 1, size, "noise").reshape(-1) for g in (0, 1)]
    for b in bufs:  # (rectangles as well: rows of the first pair's parent image)
        img = synth(5, size // 650, 650, "rects")
        b[:img.size:2] = img.reshape(-1)[::2]
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=n, **kw)
    with pkg.Context(p) as c:
        cap = c.plan(w, h)["out_capacity"]
        t = torch.from_numpy(bufs[0]).cuda()
        torch.cuda.synchronize()
        for g in (0, 1):
            if g:
                t.copy_(torch.from_numpy(bufs[1]))
                torch.cuda.synchronize()
            refs = [oracle_on(v, kw) for v in views(bufs[g])]
            # (the batches take the four result blocks in turn and a captured sequence belongs to one block: the
            # order flips every four calls so that every block sees both pairs, captured and replayed)
            for rnd in range(4):
                for k in ((0, 1, 0, 1), (1, 0, 1, 0))[rnd % 2]:
                    rs, fs = pairs[k]
                    c.batch_device(t.data_ptr() + 2, n, w, h, row_stride=rs, frame_stride=fs)
                    check(c.batch_fetch(0, n, cap), refs[k], kw["nlevels"])


def _host_entry(pkg):
    return pkg.orbx.load().orbx_detect_and_compute_batch_host


def _device_entry(pkg):
    return pkg.orbx.load().orbx_detect_and_compute_batch_device


@pytest.mark.parametrize("n,w,h,rs,gap", [(3, 643, 200, 651, 7), (1, 1241, 200, 1250, 0), (5, 250, 201, 253, 1001)])
def test_host_entry_strided(pkg, n, w, h, rs, gap):
    """orbx_detect_and_compute_batch_host with row_stride > width and frame_stride > row_stride * height: the
    hipMemcpy2DAsync branch (rows and frames packed tightly on their way to the device)."""
    kw = dict(KW["s12"], blur_levels=2)
    case = dict(name="host,%d,%d" % (w, n), kw="s12", w=w, h=h, n=n, base=0, rs=rs, fs=rs * h + gap)
    frames = case_frames(case, 0)
    refs = oracle_on(frames, kw)
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=n, **kw)
    with pkg.Context(p) as c:
        cap = c.plan(w, h)["out_capacity"]
        for fill in (0x00, 0xFF):
            buf = pack(case, frames, fill, tail=0)
            st = _host_entry(pkg)(c._h, buf.ctypes.data, n, w, h, rs, case["fs"])
            assert st == pkg.orbx.OK, st
            check(c.batch_fetch(0, n, cap), refs, kw["nlevels"])


def test_stride_argument_errors(pkg):
    """row_stride < width, a frame_stride shorter than a frame and a frame that 32-bit offsets cannot address are
    ORBX_ERR_INVALID_ARG on both entries; the context runs a correct batch afterwards."""
    import torch

    w, h, n = 643, 200, 3
    kw = dict(KW["s12"], blur_levels=2)
    case = region("errors", "s12", w, h, n, 3, 1, 653, 203)
    frames = case_frames(case, 0)
    refs = oracle_on(frames, kw)
    buf = pack(case, frames, 0xFF)
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=n, **kw)
    INV = pkg.orbx.ERR_INVALID_ARG
    with pkg.Context(p) as c:
        cap = c.plan(w, h)["out_capacity"]
        t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        dev, host = _device_entry(pkg), _host_entry(pkg)
        ptr = t.data_ptr() + case["base"]
        hptr = buf.ctypes.data + case["base"]

        def good():
            c.batch_device(ptr, n, w, h, row_stride=case["rs"], frame_stride=case["fs"])
            check(c.batch_fetch(0, n, cap), refs, kw["nlevels"])

        good()
        for rs, fs in ((w - 1, case["fs"]), (0, case["fs"]), (-653, case["fs"]),   # row_stride < width
                       (653, 653 * (h - 1) + w - 1), (653, 0), (w, w * h - 1)):    # frame_stride shorter than a frame
            assert dev(c._h, ptr, n, w, h, rs, fs, None) == INV, (rs, fs)
            assert host(c._h, hptr, n, w, h, rs, fs) == INV, (rs, fs)
            assert c._lib.orbx_last_error_string(c._h)
        # row_stride * (height - 1) + width > 2^31 - 1: the device entry refuses (nothing is read)
        assert dev(c._h, ptr, 1, w, h, 1 << 24, (1 << 24) * h, None) == INV
        assert dev(c._h, ptr, 1, w, h, (2**31 - 1 - w) // (h - 1) + 1, 1 << 40, None) == INV
        good()
        st = host(c._h, hptr, n, w, h, case["rs"], case["fs"])
        assert st == pkg.orbx.OK
        check(c.batch_fetch(0, n, cap), refs, kw["nlevels"])


# ---------------------------------------------------------------------------
# 2. frames smaller than the maximum, size changes within one context

SIZES = [(1241, 376), (1000, 300), (643, 200), (1241, 376), (1237, 371), (1241, 376)]
NSEQ = 64  # frames per batch: 1241 x 376 and 1000 x 300 then take the two passes of the top-rows-first pipeline


def sparse_frame(seed, h, w):
    """flat, with a few rectangles in the lower half only: few corners, none in the top tile rows -- so every FAST
    tile row and every pyramid row below is worked on, and whatever a denser batch left in the pools lies in the way"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 89, np.uint8)
    for _ in range(16):
        ww, hh = int(rng.integers(24, 70)), int(rng.integers(20, max(21, h // 4)))
        x0, y0 = int(rng.integers(4, w - ww - 4)), int(rng.integers(h // 2 + 4, h - hh - 4))
        img[y0:y0 + hh, x0:x0 + ww] = int(rng.choice([20, 40, 160, 230]))
    return img


_seq_cache = {}


def seq_batch(kind, w, h):
    """(frames, oracle results) of a dense (noise) or sparse batch of NSEQ frames"""
    key = (kind, w, h)
    if key not in _seq_cache:
        if kind == "dense":
            frames = np.stack([synth(9000 + 13 * i + w, h, w, "noise") for i in range(NSEQ)])
        else:
            frames = np.stack([sparse_frame(500 + 7 * i + h, h, w) for i in range(NSEQ)])
        _seq_cache[key] = (frames, oracle_on(frames, PK))
    return _seq_cache[key]


def level_counts(refs):
    return np.sum([np.bincount(r["levels"], minlength=PK["nlevels"]) for r in refs], axis=0)


def test_sequence_content_is_dense_before_and_sparse_after_a_change():
    """the precondition of the size-change tests (oracle only): on every level the batch before a size change holds
    more keypoints than the batch after it, and the sparse batches are not empty"""
    for (w0, h0), (w1, h1) in zip(SIZES, SIZES[1:]):
        dense, sparse = level_counts(seq_batch("dense", w0, h0)[1]), level_counts(seq_batch("sparse", w1, h1)[1])
        assert np.all(dense > sparse), (w0, h0, w1, h1, dense, sparse)
        assert sparse.sum() > 0


@pytest.mark.parametrize("mode", ["plain", "plain-fast-tiles", "pipelined", "pipelined-host-results", "filled-ff", "filled-55"])
def test_size_changes_within_one_context(pkg, mode, monkeypatch):
    """1241x376 -> 1000x300 -> 643x200 -> 1241x376 -> 1237x371 -> 1241x376 in one context of 1241 x 376: at every size
    a sparse batch first (right after the change), dense ones last (right before the next), three batches per size
    so that in the pipelined modes the unpipelined batch a size change forces is followed by one on each lane."""
    import torch

    if mode == "plain-fast-tiles":
        monkeypatch.setenv("ORBX_FAST_IMPL", "3")
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=NSEQ, **PK)
    dev = {}
    for w, h in set(SIZES):
        for kind in ("sparse", "dense"):
            dev[kind, w, h] = torch.from_numpy(seq_batch(kind, w, h)[0]).cuda()
    torch.cuda.synchronize()
    with pkg.Context(p) as c:
        pipelined = mode.startswith("pipelined")
        if pipelined or mode.startswith("filled"):
            c.set_pipelined_batches(True)  # (filled: so that the second lane's pools exist and are filled as well)
        if mode == "pipelined-host-results":
            c.set_host_results(True)
        fill = {"filled-ff": 0xFF, "filled-55": 0x55}.get(mode)
        for w, h in SIZES:
            cap = c.plan(w, h)["out_capacity"]
            kinds = ["sparse", "dense", "dense"]
            if not pipelined:
                for kind in kinds:
                    if fill is not None:
                        c.debug_fill_pools(fill)
                    c.batch_device(dev[kind, w, h].data_ptr(), NSEQ, w, h)
                    check(c.batch_fetch(0, NSEQ, cap), seq_batch(kind, w, h)[1])
            else:  # back to back, then the three result blocks of the ring
                for kind in kinds:
                    c.batch_device(dev[kind, w, h].data_ptr(), NSEQ, w, h)
                c.batch_prefetch()  # the whole block of the last batch (host results: the sections the kernel does not write)
                for back, kind in enumerate(reversed(kinds)):
                    hv = c.batch_host_view(previous=back)
                    check(hv, seq_batch(kind, w, h)[1], compact=hv["levels"] is None)
                    assert back == 0 or mode != "pipelined-host-results" or hv["levels"] is None


def default_fast_units(c, w, h, n):
    """units of the streaming FAST kernel's default table (tests/test_gpu_parity.py::test_fast_tile_counts)"""
    plan = c.plan(w, h)
    cols = [max(1, -(-(-(-int(x) // 4) - 2) // 62)) for x in plan["level_w"]]
    return n * sum(s * -(-int(y) // 47) for s, y in zip(cols, plan["level_h"]))


@pytest.mark.parametrize("fill", [None, 0xFF, 0x55], ids=["plain", "filled-ff", "filled-55"])
def test_adaptive_first_pass_across_a_size_change(pkg, fill):
    """The adaptive first pass re-tiles at 1241 x 376; a 1000 x 300 batch (a region of the same device frames) then
    runs with the default table of its size; back at 1241 x 376 the learning starts over from the default table and
    re-tiles again.  Every batch equals the oracle -- with `fill`, after the working pools of both lanes have been
    filled with that byte before every batch (fourth finding: nothing a skipped tile or strip left behind,
    under the old partition or the new one, is ever consumed)."""
    import torch

    n = 128
    batches = [pkg.streams.stream_a(n, first=0), pkg.streams.stream_a(n, first=256)]
    refs = [oracle_on(b, PK) for b in batches]
    w1, h1, x0, y0 = 1000, 300, 121, 37
    refs_small = oracle_on(np.ascontiguousarray(batches[0][:, y0:y0 + h1, x0:x0 + w1]), PK)
    d = [torch.from_numpy(b).cuda() for b in batches]
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=n, **PK)
    with pkg.Context(p) as c:
        cap, cap1 = c.plan(W, H)["out_capacity"], c.plan(w1, h1)["out_capacity"]
        if fill is not None:
            c.set_pipelined_batches(True)  # the second lane's pools exist and are filled as well
        base = default_fast_units(c, W, H, n)

        def learn():
            totals = []
            for i in range(10):
                if fill is not None:
                    c.debug_fill_pools(fill)
                c.batch_device(d[i & 1].data_ptr(), n, W, H)
                check(c.batch_fetch(0, n, cap), refs[i & 1])
                totals.append(c.fast_tile_counts()[1])
            assert totals[0] == base, (totals, base)  # the default table: nothing learned yet
            assert totals[-1] > totals[0], totals     # shorter tile rows: more units
            return totals

        learn()
        for _ in range(2):
            if fill is not None:
                c.debug_fill_pools(fill)
            c.batch_device(d[0].data_ptr() + y0 * W + x0, n, w1, h1, row_stride=W, frame_stride=W * H)
            check(c.batch_fetch(0, n, cap1), refs_small)
            assert c.fast_tile_counts()[1] == default_fast_units(c, w1, h1, n)
        learn()  # starts over: its first batch runs the default table again


# ---------------------------------------------------------------------------
# 3. a frame slightly smaller than the maximum whose FAST table is larger than the maximum's own


def test_tall_context_slightly_smaller_frames_top_heavy_content(pkg):
    """Context 600 x 1100, frames of 594 x 1084 with binary 2 x 2 blocks in the top tenth and flat below: the caps of
    every level fill within the first ~25 rows, the adaptive first pass asks for 16-row tile rows on every level,
    and this frame then needs 618 FAST units where the maximum's own table with such rows has 617 -- on the sizing
    before fast_tiles_upper_bound the third batch and every later one failed with ORBX_ERR_UNSUPPORTED ("FAST tile
    table exceeds pool").  Twelve batches: each succeeds and equals the oracle, and the table did change, to the
    partition that pool could not hold."""
    import torch

    wm, hm, w, h, n = 600, 1100, 594, 1084, 32
    batches = []
    for b in range(2):
        fr = np.full((n, h, w), 89, np.uint8)
        for i in range(n):
            rng = np.random.default_rng(300 + 50 * b + i)
            blocks = rng.integers(0, 2, (h // 20 + 1, w // 2 + 1), dtype=np.uint8) * 255
            fr[i, :h // 10] = np.kron(blocks, np.ones((2, 2), np.uint8))[:h // 10, :w]
        batches.append(fr)
    refs = [oracle_on(b, PK) for b in batches]
    d = [torch.from_numpy(b).cuda() for b in batches]
    torch.cuda.synchronize()
    p = pkg.default_params("gpu", max_width=wm, max_height=hm, max_batch=n, **PK)
    with pkg.Context(p) as c:
        cap = c.plan(w, h)["out_capacity"]
        totals = []
        for i in range(12):
            c.batch_device(d[i & 1].data_ptr(), n, w, h)  # (an overflowing table is an error code of this call)
            check(c.batch_fetch(0, n, cap), refs[i & 1], PK["nlevels"])
            totals.append(c.fast_tile_counts()[1])
        assert totals[0] == default_fast_units(c, w, h, n), totals
        assert len(set(totals)) > 1 and max(totals) > totals[0], totals
        assert max(totals) >= 618 * n, totals  # (617 units per frame: what the maximum's own 16-row table has)


def test_zz_report():
    """(last in the module: how many (case, frame) comparisons the module made -- DESIGN.md §3 quotes it)"""
    print("test_batch_inputs: %d (case, frame) comparisons against the oracle" % COMPARISONS[0])
    assert COMPARISONS[0] > 0
