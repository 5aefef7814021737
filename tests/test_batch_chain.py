"""The batched chain  batch -> match -> pose -> scale  on uneven batches, against the CPU chain of tests/chain_ref.py
("uneven batches").

Every stage of the chain indexes the previous stage's tables by per-frame counts that live on the device, in rows of
out_capacity slots, in one set of buffers per context that is never cleared between batches.  The other GPU tests of
the chain feed it the two KITTI fixtures alternating: equal query and train counts, no empty frame, hundreds of
matches per pair, rows as long as the ones the previous batch left.  Here the batches hold what those do not:

  set U  rich, empty and nearly empty frames next to each other, pairs with 0, 1-4, 5-63 (with and without a model),
         64-255 and more matches, joins after a zero pose, joins without a ratio, clamped scales;
  set Q  keypoint counts at wave and workgroup boundaries (64, 255, 256, 257, 2047, 2048);
  set S  set U at smaller sizes in a context of 1241 x 376, and in a strided device buffer;
  set H  1920 x 1080, 12 levels, 4000 features, with an empty frame in the middle.

The CPU tests (no marker) assert from the CPU chain alone that the sets hold these classes, and print the tables that
DESIGN.md quotes.  The GPU tests compare everything the context offers with the chain: exact equality, no tolerance.

Measured on the MI355X when the file was written: DESIGN.md §9, "uneven batches".
"""
import ctypes as C

import numpy as np
import pytest

import chain_ref as R
from chain_ref import H, K_1080, K_KITTI, OKW_H, OKW_U, W
from test_batch_inputs import pack, region
from test_scale import pose_seq, seq  # noqa: F401  (fixtures: the two restatements, compiled per module)

SEED64 = 0x9E3779B97F4A7C15
# (prob, threshold, max_iters, seed): combinations of gpu_cases() in tests/test_pose.py, through the batched entry
RANSAC_ARGS = [(0.99, 0.5, 7, SEED64), (0.5, 2.0, 1, SEED64), (0.999, 1.0, 1000, SEED64), (0.99, 2.0, 1000, 2654435761)]


@pytest.fixture(scope="module")
def libs(pose_seq, seq):  # noqa: F811
    return pose_seq, seq


def matches(p):
    return len(p["q"])


# ---- CPU: the sets are what they claim ------------------------------------------------------


def test_cpu_set_u_classes(libs):
    frames = R.set_u()
    ref = R.chain(libs, frames, OKW_U)
    print("set U (%d frames)\n%s" % (len(frames), R.table(ref)))
    P = ref["pairs"]
    it = R.POSE_DEFAULTS["max_iters"]

    def some(f):
        return any(f(p) for p in P)

    assert some(lambda p: p["nq"] == 0)
    assert some(lambda p: 0 < p["nq"] < 64)
    assert some(lambda p: p["nq"] > 256 and p["nq"] != p["nt"])
    assert some(lambda p: p["nt"] == 0 and p["nq"] > 0)
    assert some(lambda p: matches(p) == 0 and p["nq"] > 0 and p["nt"] > 0)
    assert some(lambda p: 1 <= matches(p) <= 4)
    assert some(lambda p: 5 <= matches(p) <= 63 and p["pose"]["inliers"] > 0)
    assert some(lambda p: 5 <= matches(p) <= 63 and p["pose"]["iters"] == it and R.is_zero_pose(p))
    assert some(lambda p: 64 <= matches(p) < 256)
    assert some(lambda p: matches(p) >= 256)
    joined = [(a, b) for a, b in zip(P, P[1:]) if b["triplets"] > 0]
    assert any(matches(a) < matches(b) for a, b in joined) and any(matches(a) > matches(b) for a, b in joined)
    # a join after a zero pose (R = I, t = 0), one of them after five or more matches without a model
    assert any(R.is_zero_pose(a) for a, b in joined)
    assert any(R.is_zero_pose(a) and matches(a) >= 5 for a, b in joined)
    assert any(R.is_zero_pose(a) and b["ratios"] > 0 for a, b in joined)
    # triplets without a single ratio; a scale clamped at either end
    assert some(lambda p: p["triplets"] > 0 and p["ratios"] == 0 and p["scale"] == 1.0)
    assert some(lambda p: p["ratios"] > 0 and p["scale"] == 0.1)
    assert some(lambda p: p["ratios"] > 0 and p["scale"] == 5.0)
    assert some(lambda p: p["ratios"] > 0 and 0.1 < p["scale"] < 5.0)
    assert len(ref["frames"][0]["kps"]) > 0 and len(ref["frames"][-1]["kps"]) > 0
    # the same frames in another order: empty frames first and last
    var = R.set_u_flat_ends()
    assert len(var) == len(frames)
    vref = R.chain(libs, var, OKW_U)
    print("set U, flat ends\n%s" % R.table(vref))
    assert len(vref["frames"][0]["kps"]) == 0 and len(vref["frames"][-1]["kps"]) == 0
    assert any(matches(p) >= 256 for p in vref["pairs"]) and any(0 < matches(p) < 64 for p in vref["pairs"])


def test_cpu_set_q_counts(libs):
    for nf, count in R.Q_NFEATURES.items():
        ref = R.chain(libs, R.set_q(), dict(nfeatures=nf))
        print("set Q, nfeatures %d\n%s" % (nf, R.table(ref)))
        assert [len(r["kps"]) for r in ref["frames"]] == [count] * 3, nf
        assert all(matches(p) >= 5 for p in ref["pairs"]), nf


def test_cpu_set_s_classes(libs):
    for w, h in R.S_SIZES:
        ref = R.chain(libs, R.set_s(w, h), OKW_U)
        print("set S, %d x %d\n%s" % (w, h, R.table(ref)))
        assert any(len(r["kps"]) == 0 for r in ref["frames"]), (w, h)
        assert any(1 <= matches(p) <= 63 for p in ref["pairs"]), (w, h)
        assert any(matches(p) >= 64 for p in ref["pairs"]), (w, h)


def test_cpu_set_h_classes(pkg, libs):
    ref = R.chain(libs, R.set_h(pkg), OKW_H, K_1080)
    print("set H\n%s" % R.table(ref))
    counts = [len(r["kps"]) for r in ref["frames"]]
    assert all(counts[i] > 3000 for i in (0, 1, 3, 4)) and counts[2] == 0, counts
    m = [matches(p) for p in ref["pairs"]]
    assert m[0] > 2048 and m[3] > 2048 and m[1] == 0 and m[2] == 0, m


# ---- GPU ------------------------------------------------------------------------------------


def params(pkg, okw, max_batch, w=W, h=H):
    return pkg.default_params("gpu", max_width=w, max_height=h, max_batch=max_batch, **okw)


def run_and_check(c, libs, frames, okw, K=K_KITTI, ratio=0.8, **pose_kw):
    """the frames through all four stages, then everything against the CPU chain"""
    h, w = frames[0].shape
    c.batch_host(np.stack(frames))
    R.run_chain(c, K, ratio, **pose_kw)
    ref = R.chain(libs, frames, okw, K, ratio, **pose_kw)
    assert R.check(c, ref, w, h) == len(frames) - 1
    return ref


def pair_bits(c, pair, cap):
    """everything fetched for one pair, as comparable values"""
    po, sc = c.batch_pose_fetch(pair, 1), c.batch_scale_fetch(pair, 1)
    xyz, valid = c.batch_points_fetch(pair)
    return ([a.tobytes() for a in c.batch_match_fetch(pair, cap)], [po[k].tobytes() for k in sorted(po)],
            c.batch_pose_mask(pair).tobytes(), xyz.tobytes(), valid.tobytes(), [sc[k].tobytes() for k in sorted(sc)])


@pytest.mark.gpu
def test_gpu_set_u(pkg, libs):
    """Set U in a context whose max_batch is exactly its length; the same frames in the order with empty frames
    first and last; the same frames at two positions of one batch give the same bits."""
    frames = R.set_u()
    with pkg.Context(params(pkg, OKW_U, len(frames))) as c:
        cap = c.plan(W, H)["out_capacity"]
        run_and_check(c, libs, frames, OKW_U)
        # k0 -> k1 -> k0 -> k1 at frames 12-15 and k0 -> k1 at frames 0-1: pairs 0, 12 and 14 see the same frames (the
        # scale of a pair depends on its predecessor as well: pairs 0 and 12 differ there)
        a, b, d = pair_bits(c, 0, cap), pair_bits(c, 12, cap), pair_bits(c, 14, cap)
        assert a[:5] == b[:5] == d[:5]
        run_and_check(c, libs, R.set_u_flat_ends(), OKW_U)
        run_and_check(c, libs, frames, OKW_U)


@pytest.mark.gpu
def test_gpu_stale_tables(pkg, libs):
    """One context: a rich batch (k0, k1 alternating, max_batch frames) through all stages, then set U, then the rich
    batch again.  No row of the match, pose, point and scale tables of the second run is longer than what the first
    left there, and all but the four k0 / k1 pairs of set U are far shorter; nothing is cleared in between."""
    frames = R.set_u()
    n = len(frames)
    with pkg.Context(params(pkg, OKW_U, n)) as c:
        rich = run_and_check(c, libs, R.rich(n), OKW_U)
        ref = run_and_check(c, libs, frames, OKW_U)
        assert all(matches(p) <= matches(r) for p, r in zip(ref["pairs"], rich["pairs"]))
        assert sum(matches(p) < matches(r) for p, r in zip(ref["pairs"], rich["pairs"])) >= n - 5
        run_and_check(c, libs, R.rich(n), OKW_U)
        run_and_check(c, libs, R.set_u_flat_ends(), OKW_U)


@pytest.mark.gpu
@pytest.mark.parametrize("host_results", [False, True], ids=["pipelined", "pipelined-host-results"])
def test_gpu_set_u_lanes(pkg, libs, host_results):
    """Pipelined batches: a rich batch matched and posed on the other lane first (the pattern of
    test_gpu_pose_lanes_and_invalid_states), then set U; with and without results written to the host mirror."""
    frames = R.set_u()
    k0, k1 = frames[0], frames[1]
    with pkg.Context(params(pkg, OKW_U, len(frames))) as c:
        c.set_pipelined_batches(True)
        if host_results:
            c.set_host_results(True)
        c.batch_host(np.stack([k1, k0, k1, k1]))  # another batch first, on the other lane
        c.batch_match_consecutive(0.8)
        c.batch_pose_consecutive(K_KITTI)
        run_and_check(c, libs, frames, OKW_U)
        run_and_check(c, libs, R.set_u_flat_ends(), OKW_U)  # the other lane
        run_and_check(c, libs, R.rich(len(frames)), OKW_U)
        run_and_check(c, libs, frames, OKW_U)


@pytest.mark.gpu
def test_gpu_batched_ransac_arguments_and_ratios(pkg, libs):
    """Non-default prob, threshold, max_iters and a 64-bit seed through the batched entry, and ratios other than 0.8
    through the batched matcher, on set U and on set Q at 256 keypoints per frame."""
    for frames, okw in ((R.set_u(), OKW_U), (R.set_q(), dict(nfeatures=260))):
        with pkg.Context(params(pkg, okw, len(frames))) as c:
            for prob, thr, iters, seed in RANSAC_ARGS:
                run_and_check(c, libs, frames, okw, prob=prob, threshold=thr, max_iters=iters, seed=seed)
            for ratio in (0.7, 1.0):
                run_and_check(c, libs, frames, okw, ratio=ratio)
            run_and_check(c, libs, frames, okw, ratio=0.7, prob=0.99, threshold=0.5, max_iters=7, seed=SEED64)


@pytest.mark.gpu
@pytest.mark.parametrize("nfeatures", sorted(R.Q_NFEATURES))
def test_gpu_set_q(pkg, libs, nfeatures):
    okw = dict(nfeatures=nfeatures)
    with pkg.Context(params(pkg, okw, 3)) as c:
        ref = run_and_check(c, libs, R.set_q(), okw)
    assert [len(r["kps"]) for r in ref["frames"]] == [R.Q_NFEATURES[nfeatures]] * 3


@pytest.mark.gpu
def test_gpu_set_s_sizes_within_one_context(pkg, libs):
    """full-size rich -> 1000 x 300 -> 643 x 200 -> full-size set U -> 1237 x 371 -> full-size rich in one context of
    1241 x 376: match, pose and scale take their row pitch from the plan of the moment."""
    n = len(R.set_u())
    with pkg.Context(params(pkg, OKW_U, n)) as c:
        run_and_check(c, libs, R.rich(n), OKW_U)
        run_and_check(c, libs, R.set_s(1000, 300), OKW_U)
        run_and_check(c, libs, R.set_s(643, 200), OKW_U)
        run_and_check(c, libs, R.set_u(), OKW_U)
        run_and_check(c, libs, R.set_s(1237, 371), OKW_U)
        run_and_check(c, libs, R.rich(n), OKW_U)


@pytest.mark.gpu
def test_gpu_set_u_strided_device_batch(pkg, libs):
    """Set U as regions of a larger device buffer: row_stride > width, a gap between the frames, an odd base."""
    import torch

    frames = R.set_u()
    n = len(frames)
    case = region("set-u", None, W, H, n, 3, 2, 1251, 380)
    ref = R.chain(libs, frames, OKW_U)
    with pkg.Context(params(pkg, OKW_U, n)) as c:
        for fill in (0x00, 0xFF):
            t = torch.from_numpy(pack(case, np.stack(frames), fill)).cuda()
            torch.cuda.synchronize()
            c.batch_device(t.data_ptr() + case["base"], n, W, H, row_stride=case["rs"], frame_stride=case["fs"])
            R.run_chain(c)
            assert R.check(c, ref) == n - 1


@pytest.mark.gpu
def test_gpu_set_h(pkg, libs):
    frames = R.set_h(pkg)
    with pkg.Context(params(pkg, OKW_H, len(frames), 1920, 1080)) as c:
        assert c.plan(1920, 1080)["out_capacity"] >= 4000
        for _ in range(2):
            run_and_check(c, libs, frames, OKW_H, K_1080)


@pytest.mark.gpu
def test_gpu_batch_shapes(pkg, libs):
    """Two frames (one pair) in a context of two; set U in a context of twice its length."""
    frames = R.set_u()
    with pkg.Context(params(pkg, OKW_U, 2)) as c:
        for pair in ((0, 1), (1, 2), (4, 5), (5, 6), (6, 7), (7, 8), (9, 10), (10, 11)):
            run_and_check(c, libs, [frames[pair[0]], frames[pair[1]]], OKW_U)
    with pkg.Context(params(pkg, OKW_U, 2 * len(frames))) as c:
        run_and_check(c, libs, frames, OKW_U)
        run_and_check(c, libs, frames + R.set_u_flat_ends(), OKW_U)
        run_and_check(c, libs, frames[3:9], OKW_U)


@pytest.mark.gpu
def test_gpu_fetch_edges_on_a_pair_without_matches(pkg, libs):
    """batch_match_fetch, batch_pose_mask and batch_points_fetch with capacity 0 succeed with count 0 on a pair with
    zero matches (NULL outputs); batch_pose_fetch of that pair returns the zero result exactly."""
    frames = R.set_u()
    lib = pkg.orbx.load()
    with pkg.Context(params(pkg, OKW_U, len(frames))) as c:
        ref = run_and_check(c, libs, frames, OKW_U)
        empty = [i for i, p in enumerate(ref["pairs"]) if matches(p) == 0]
        assert len(empty) >= 4
        for pair in empty:
            for call in (lambda n: lib.orbx_batch_match_fetch(c._h, pair, None, None, None, 0, n),
                         lambda n: lib.orbx_batch_pose_mask(c._h, pair, None, 0, n),
                         lambda n: lib.orbx_batch_points_fetch(c._h, pair, None, None, 0, n)):
                cnt = C.c_int(-1)
                assert call(C.byref(cnt)) == pkg.orbx.OK and cnt.value == 0, pair
            r = c.batch_pose_fetch(pair, 1)
            assert r["E"].tobytes() == np.zeros((1, 3, 3)).tobytes() and r["R"].tobytes() == np.eye(3)[None].tobytes()
            assert r["t"].tobytes() == np.zeros((1, 3)).tobytes()
            assert (int(r["inliers"][0]), int(r["good"][0]), int(r["iters"][0])) == (0, 0, 0)
            s = c.batch_scale_fetch(pair, 1)
            assert (s["scale"][0], int(s["triplets"][0]), int(s["ratios_used"][0])) == (1.0, 0, 0)
        # a pair with matches and capacity 0: the count comes back with ORBX_ERR_CAPACITY
        cnt = C.c_int(-1)
        assert lib.orbx_batch_match_fetch(c._h, 0, None, None, None, 0, C.byref(cnt)) == pkg.orbx.ERR_CAPACITY
        assert cnt.value == matches(ref["pairs"][0])
        R.check(c, ref)  # the refused fetches changed nothing
