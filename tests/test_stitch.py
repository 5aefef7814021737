"""GPU tests of the stream path (include/orbx_stream.h).  The rule throughout: the new route has
to equal the existing route fed with the fetched intermediates, bit for bit.

  stitch  orbx_stitch_windows_device on uploaded poses == tests/cpp/st_sequential.cpp
  chain   orbx_window_poses_stream_device == orbx_window_poses_device with T0 = NULL and the scale0 the host assembles
          from orbx_tracks_pose_fetch by the rule
  stream  orbx_stream_odometry_tracks_device == the six stages called one by one, every stage's block and the
          trajectory; the host twin gives the same bits; the trajectory against numpy and against the true path
  state   another stream than the write-back's, refusals, growth, and the other side paths' blocks stay untouched
"""
import ctypes as C

import numpy as np
import pytest

import landmarks_ref as LR
import stitch_ref as R
import stitch_seq as SS
import tracks_pose_ref as T

pytestmark = pytest.mark.gpu
CASES = {cs["name"]: cs for cs in R.cases()}
TP_CASES = {cs["name"]: cs for cs in T.gpu_cases()}
STREAM = dict(W=3, L=5, stride=2)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return SS.compile_seq(tmp_path_factory.mktemp("st_seq_gpu"))


@pytest.fixture()
def streams(pkg):
    hip = pkg.orbx.load()
    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    yield sa.value, sb.value
    assert hip.hipStreamDestroy(sa) == 0 and hip.hipStreamDestroy(sb) == 0


def upload(*arrays):
    import torch

    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def flat(x):
    if isinstance(x, dict):
        return [(k, flat(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [flat(a) for a in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def start_pose(seed):
    rng = np.random.default_rng(seed)
    return R.WR.rigid(R.WR.rot(rng.normal(size=3), 0.8), rng.normal(size=3) * 4.0)


# ---- 1. stitch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_stitch_equals_the_sequential_restatement(pkg, ctx, seq, name, given):
    S, cs = pkg.orbx_stream, CASES[name]
    W, L = cs["poses"].shape[:2]
    stride, T0 = cs["stride"], cs["T_start"] if given else None
    (poses,) = upload(cs["poses"])
    for align in ((False, True) if stride <= L - 2 else (False,)):
        S.stitch_windows_device(ctx, poses, stride, T0, align)
        got = S.stitch_fetch(ctx)
        SS.assert_stitch_equal(got, SS.seq_stitch(seq, cs["poses"], stride, T0, align))
        SS.assert_stitch_equal(got, S.stitch_windows(cs["poses"], stride, T0, align))  # the host twin
    F = R.frames(W, L, stride)
    v = S.stitch_view(ctx)
    assert (v.n_frames, v.n_windows, v.window_len, v.stride) == (F, W, L, stride)
    assert v.trajectory4x4 and v.owner and v.anchors4x4 and getattr(v, "lambda") and v.status
    # ranges of the block are slices of the whole
    f0, w0 = F // 2, W - 1
    part = S.stitch_fetch(ctx, f0, F - f0, w0, 1)
    for k in SS.KEYS:
        whole = got[k][f0:] if k in ("trajectory4x4", "owner") else got[k][w0:]
        assert SS.bits_equal(part[k], whole), k
    first = S.stitch_fetch(ctx, 0, 1, 0, 1)
    assert all(SS.bits_equal(first[k], got[k][:1]) for k in SS.KEYS)


def test_the_shapes_cross_the_block_edges():
    """W = 65 and 130 cross the 64-lane block of the per-window kernels, F = 197, 911 and 782 that of the per-frame
    kernel, each with a last block that is not full"""
    F = sorted(R.frames(*s) for s in R.SHAPES)
    assert F == [2, 4, 8, 13, 197, 782, 911] and all(f % 64 for f in F)
    assert sorted(s[0] for s in R.SHAPES) == [1, 2, 5, 7, 65, 130, 130]


def test_a_broken_window_on_the_device(pkg, ctx, seq):
    S, cs = pkg.orbx_stream, CASES["W65_L5_s3_scaled"]
    poses = cs["poses"].copy()
    poses[63, 1, 0, 3], poses[64, 0, 2, 2] = np.nan, np.inf  # either side of the block edge
    S.stitch_windows_device(ctx, poses, cs["stride"], cs["T_start"], True)
    got = S.stitch_fetch(ctx)
    SS.assert_stitch_equal(got, SS.seq_stitch(seq, poses, cs["stride"], cs["T_start"], True))
    assert got["status"][62:65].tolist() == [R.OK, R.BROKEN, R.BROKEN] and np.isfinite(got["trajectory4x4"]).all()


# ---- 2. the stream's chain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TP_CASES))
def test_stream_chain_equals_the_chain_with_the_host_scale0(pkg, ctx, seq, name):
    S, VO, cs = pkg.orbx_stream, pkg.orbx_vo, TP_CASES[name]
    n, L = len(cs["seen"]), cs["L"]
    t, s = upload(cs["tracks"], cs["seen"])
    ctx.tracks_pose(cs["K"], t, s, **cs["kw"])
    scale = ctx.tracks_pose_fetch()["scale"].reshape(n, L - 1)
    assert np.isfinite(scale).all()
    for stride in sorted({1, max(L - 2, 1), L - 1}):
        first = 0.5 + stride
        S.window_poses_stream(ctx, stride, first)
        got = VO.window_poses_fetch(ctx)
        s0 = np.ones(n)
        s0[0] = first
        if stride <= L - 2:
            s0[1:] = scale[:-1, stride]
        assert SS.bits_equal(SS.seq_scale0(seq, scale, stride, first), s0)
        VO.window_poses(ctx, None, s0)
        want = VO.window_poses_fetch(ctx)
        assert all(SS.bits_equal(got[k], want[k]) for k in ("poses6", "poses4x4", "status")), stride
        assert (got["poses4x4"][:, 0] == np.eye(4)).all()


def test_the_chain_cases_have_the_window_lengths_and_scales_they_need(ctx):
    assert sorted({cs["L"] for cs in TP_CASES.values()}) == [2, 3, 5]
    cs = TP_CASES["cap257"]
    ctx.tracks_pose(cs["K"], *upload(cs["tracks"], cs["seen"]), **cs["kw"])
    scale = ctx.tracks_pose_fetch()["scale"].reshape(len(cs["seen"]), cs["L"] - 1)
    assert (scale[:-1, 1:] != 1.0).any()  # a gathered scale that is not the default


# ---- 3. the stream entry ------------------------------------------------------------------------------------------------
def stage_blocks(pkg, c, views):
    out = dict(tp=c.tracks_pose_fetch(), wp=pkg.orbx_vo.window_poses_fetch(c), lm=c.landmarks_fetch(),
               ba=c.bundle_adjust_landmarks_fetch(), wb=pkg.orbx_vo.bundle_adjust_write_back_fetch(c),
               st=pkg.orbx_stream.stitch_fetch(c))
    if views:
        out["lmv"] = pkg.orbx_lm.landmarks_views_fetch(c)
    return out


def one_by_one(pkg, c, sc, t, s, T0, views, stream_of=lambda i: None):
    S, VO, LM = pkg.orbx_stream, pkg.orbx_vo, pkg.orbx_lm
    c.tracks_pose(sc["K"], t, s, stream=stream_of(0))
    S.window_poses_stream(c, STREAM["stride"], 1.0, stream=stream_of(1))
    if views:
        LM.landmarks_build_views(c, sc["K"], t, s, None, LM.TRI_ALL_VIEWS, 3.0, stream=stream_of(2))
    else:
        VO.landmarks_build_chained(c, sc["K"], t, s, stream=stream_of(2))
    c.bundle_adjust_landmarks(stream=stream_of(3))
    VO.bundle_adjust_write_back(c, stream=stream_of(4))
    S.stitch_windows_device(c, VO.bundle_adjust_write_back_view(c), STREAM["stride"], T0, True, stream=stream_of(5))


@pytest.mark.parametrize("slots,views", [(63, False), (65, False), (65, True)])
def test_stream_entry_equals_the_stages_one_by_one(pkg, ctx, slots, views):
    S, LM = pkg.orbx_stream, pkg.orbx_lm
    sc = R.scene_stream(slots=slots, seed=300 + slots, **STREAM)
    T0 = start_pose(slots)
    t, s = upload(sc["tracks"], sc["seen"])
    options = dict(tri_mode=LM.TRI_ALL_VIEWS, max_reproj_px=3.0) if views else {}
    S.stream_odometry_tracks_device(ctx, sc["K"], t, s, stride=STREAM["stride"], T_start=T0, align_scale=True, **options)
    got = stage_blocks(pkg, ctx, views)
    if not views:
        with pytest.raises(pkg.OrbxError):  # the reference's build leaves no views diagnostics
            LM.landmarks_views_fetch(ctx)
    one_by_one(pkg, ctx, sc, t, s, T0, views)
    want = stage_blocks(pkg, ctx, views)
    for k in want:
        assert flat(got[k]) == flat(want[k]), k
    # the windows are solved, and the stream is joined
    st = got["st"]
    assert (got["lm"]["status"] == LR.OK).all() and (st["status"] == R.OK).all()
    assert all(sm["termination"] == pkg.orbx.BA_CONVERGENCE for sm in got["ba"][1])
    assert len(st["trajectory4x4"]) == R.frames(**STREAM) and SS.bits_equal(st["anchors4x4"][0], T0)
    # against numpy on the fetched write-back poses, with the bound of stitch_ref
    wb = got["wb"][0]
    case = dict(poses=wb, T_start=T0)
    ref = R.stitch(wb, STREAM["stride"], T0, True, np.longdouble)
    d, tol = R.distance(st, ref), R.tolerance(case, ref)
    print("slots %d: distance to numpy in longdouble %.3e, tolerance %.3e" % (slots, d, tol))
    assert d <= tol and np.array_equal(st["owner"], ref["owner"])
    # the true path up to one global similarity: no further from it than the numpy route is, within that bound
    got_c, got_a = R.similarity_residual(st["trajectory4x4"], sc["true"])
    ref_c, ref_a = R.similarity_residual(ref["trajectory4x4"].astype(np.float64), sc["true"])
    print("slots %d: residual to the true path %.3e units, %.3e rad (numpy: %.3e, %.3e)" % (slots, got_c, got_a, ref_c,
                                                                                            ref_a))
    assert got_c <= ref_c + tol and got_a <= ref_a + tol
    # the host twin
    twin = S.stream_odometry_tracks(ctx, sc["K"], sc["tracks"], sc["seen"], STREAM["stride"], T0, align_scale=True,
                                    **options)
    assert SS.bits_equal(twin["trajectory4x4"], st["trajectory4x4"])
    assert np.array_equal(twin["st_status"], st["status"]) and np.array_equal(twin["wp_status"], got["wp"]["status"])
    assert np.array_equal(twin["lm_status"], got["lm"]["status"]) and twin["summaries"] == got["ba"][1]
    for k in want:
        assert flat(stage_blocks(pkg, ctx, views)[k]) == flat(want[k]), k


def test_the_stitch_waits_for_a_write_back_on_another_stream(pkg, streams):
    """every stage on the next caller stream, the stitch reading the write-back view on another stream than the
    write-back ran on, no host wait in between: the same-stream result"""
    S = pkg.orbx_stream
    sc = R.scene_stream(slots=65, seed=365, **STREAM)
    T0 = start_pose(5)
    order = list(streams) + [None]
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        t, s = upload(sc["tracks"], sc["seen"])
        one_by_one(pkg, c, sc, t, s, T0, False)
        same = flat(stage_blocks(pkg, c, False))
        for shift in (0, 1):
            one_by_one(pkg, c, sc, t, s, T0, False, stream_of=lambda i: order[(i + shift) % 3])
            assert flat(stage_blocks(pkg, c, False)) == same, shift
        # the window-poses view on another stream than the chain's
        S.window_poses_stream(c, STREAM["stride"], 1.0, stream=order[0])
        S.stitch_windows_device(c, pkg.orbx_vo.window_poses_view(c), STREAM["stride"], T0, True, stream=order[1])
        got = S.stitch_fetch(c)
        SS.assert_stitch_equal(got, S.stitch_windows(pkg.orbx_vo.window_poses_fetch(c)["poses4x4"], STREAM["stride"],
                                                     T0, True))


# ---- 4. state -------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(pkg):
    S, VO = pkg.orbx_stream, pkg.orbx_vo
    sc = R.scene_stream(slots=40, seed=77, **STREAM)
    T0 = start_pose(6)
    bad_T = T0.copy()
    bad_T[0, 3] = np.inf
    INVALID = pkg.orbx.ERR_INVALID_ARG

    def refused(call):
        with pytest.raises(pkg.OrbxError) as e:
            call()
        assert e.value.status == INVALID

    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        for call in (lambda: S.stitch_fetch(c), lambda: S.stitch_view(c), lambda: S.window_poses_stream(c, 1)):
            refused(call)  # nothing stitched, nothing to chain
        t, s = upload(sc["tracks"], sc["seen"])
        S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, T_start=T0, align_scale=True)
        others = lambda: flat((c.tracks_pose_fetch(), VO.window_poses_fetch(c), c.landmarks_fetch(),
                               c.bundle_adjust_landmarks_fetch(), VO.bundle_adjust_write_back_fetch(c)))
        before, kept = flat(S.stitch_fetch(c)), others()
        wb = VO.bundle_adjust_write_back_view(c)
        L = STREAM["L"]
        for call in (
                lambda: S.stitch_windows_device(c, wb, 0), lambda: S.stitch_windows_device(c, wb, L),
                lambda: S.stitch_windows_device(c, wb, L - 1, None, True),
                lambda: S.stitch_windows_device(c, None, 2, n_windows=3, window_len=L),
                lambda: S.stitch_windows_device(c, wb, 2, bad_T),
                lambda: S.stitch_windows_device(c, wb.poses4x4, 2, n_windows=0, window_len=L),
                lambda: S.window_poses_stream(c, 0), lambda: S.window_poses_stream(c, L),
                lambda: S.window_poses_stream(c, 2, np.nan),
                lambda: S.stitch_fetch(c, 0, R.frames(**STREAM) + 1), lambda: S.stitch_fetch(c, 0, 1, 2, 2),
                # the stream entry: an argument any stage would refuse, before the first launch
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=L, T_start=T0),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=L - 1, align_scale=True),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, T_start=bad_T),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, scale0_first=np.inf),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, prob=np.nan),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, tri_mode=3),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, max_reproj_px=-1.0),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, ba_max_iters=0),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t, s, stride=2, max_rot=0.0),
                lambda: S.stream_odometry_tracks_device(c, sc["K"], t.data_ptr(), None, stride=2, n_windows=3,
                                                        slot_capacity=40, window_len=L),
                lambda: S.stream_odometry_tracks(c, sc["K"], sc["tracks"], sc["seen"], L, T0)):
            refused(call)
            assert flat(S.stitch_fetch(c)) == before and others() == kept
        # a stitch changes no other path's block
        S.stitch_windows_device(c, wb, 1)
        assert flat(S.stitch_fetch(c)) != before and others() == kept


def test_growth_and_back(pkg, seq):
    S = pkg.orbx_stream
    small, large = CASES["W2_L3_s1_scaled"], CASES["W130_L8_s6_scaled"]
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        for cs in (small, large, small):
            S.stitch_windows_device(c, cs["poses"], cs["stride"], cs["T_start"], True)
            SS.assert_stitch_equal(S.stitch_fetch(c), SS.seq_stitch(seq, cs["poses"], cs["stride"], cs["T_start"], True))
            v = S.stitch_view(c)
            assert (v.n_windows, v.n_frames) == (len(cs["poses"]), len(cs["true"]))
