"""Landmarks built on the device from every view of a track, with the reprojection gate and its diagnostics
(include/orbx_lm.h).  The landmarks block, reason and reproj_px are compared bit for bit with the
sequential restatement tests/cpp/lm_views_sequential.cpp; the first-two build without a gate byte for byte with
orbx_landmarks_build_device / orbx_landmarks_build_chained_device; the solve behind an all-views block bit for bit with
orbx_bundle_adjust_batch on the fetched arrays.  Synthetic tracks are uploaded as tensors: no images but in the stream
and the untouched-results tests."""
import ctypes as C

import numpy as np
import pytest

import landmarks_ref as R
import landmarks_seq as S
import landmarks_views_seq as VS
import oracle_lib as O
import tracks_pose_ref as T
from test_landmarks import K_CROP, check_solve, u64

pytestmark = pytest.mark.gpu
K = R.K_KITTI
GATES = (0.0, 3.0)
SHAPES = [(5, 2), (63, 3), (257, 5), (63, 8)]  # (slot capacity, window length)
CASES = {c["name"]: c for c in T.gpu_cases()}  # tracked windows whose poses the device chains (rank 14)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("lm_views_seq_gpu"), "lm_views_sequential")


def upload(*arrays):
    import torch

    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def gpu_views(pkg, ctx, scenes, mode, gate, **kw):
    """(block, reason, reproj_px) of a views build of the scenes"""
    poses, tracks, seen = R.stack(scenes)
    pkg.orbx_lm.landmarks_build_views(ctx, K, tracks, seen, poses, mode, gate, **kw)
    return (ctx.landmarks_fetch(),) + pkg.orbx_lm.landmarks_views_fetch(ctx)


def assert_views_equal(got, ref):
    S.assert_blocks_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))


def mixed_scenes(slots, W):
    """noisy, tilted and with outliers | baseline-gated | all behind | a pose beyond 1e5 rad past the first two (the
    last pose of a window shorter than 4) | ragged with short tracks"""
    ok = R.make_scene(401, W=W, slots=slots, min_seen=0, world=R.WORLD_TILTED, sigma=0.3, outliers=0.1, pose_pert=0.002)
    baseline = R.make_scene(402, W=W, slots=slots, min_seen=2, step=0.05)
    behind = R.make_scene(403, W=W, slots=slots, min_seen=1, depth_sign=-1.0)
    bad = R.make_scene(404, W=W, slots=slots, min_seen=2)
    bad["poses"][min(3, W - 1), :3] = np.array([0.0, 2e5, 0.0])
    ragged = R.make_scene(405, W=W, slots=slots, min_seen=0, sigma=0.3, outliers=0.3)
    return [ok, baseline, behind, bad, ragged]


# ---- 1. the first-two build without a gate is the build of rank 10 --------------------------------------------------
@pytest.mark.parametrize("slots,W", SHAPES)
def test_first_two_without_a_gate_equals_the_plain_build(pkg, ctx, slots, W):
    scenes = mixed_scenes(slots, W)
    poses, tracks, seen = R.stack(scenes)
    ctx.landmarks_build(K, tracks, seen, poses)
    plain = ctx.landmarks_fetch()
    got, reason, px = gpu_views(pkg, ctx, scenes, VS.FIRST_TWO, 0.0)
    assert list(plain["status"][1:3]) == [R.BASELINE, R.EMPTY] and sorted(got) == sorted(plain)
    assert slots < 63 or plain["status"][0] == R.OK
    for k in plain:
        assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k
    kept = np.zeros((len(scenes), slots), bool)
    for w in range(len(scenes)):
        kept[w, S.window_of(plain, w)[1]] = True
    assert np.array_equal(reason == VS.KEPT, kept)


def test_first_two_without_a_gate_equals_the_chained_build(pkg, ctx):
    VO, LM = pkg.orbx_vo, pkg.orbx_lm
    for name in ("cap63", "cap257"):
        cs = CASES[name]
        t_dev, s_dev = upload(cs["tracks"], cs["seen"])
        ctx.tracks_pose(cs["K"], t_dev, s_dev, **cs["kw"])
        VO.window_poses(ctx)
        VO.landmarks_build_chained(ctx, cs["K"], t_dev, s_dev)
        chained = ctx.landmarks_fetch()
        assert name != "cap257" or ((chained["status"] == R.OK).sum() >= 3 and chained["point_offset"][-1] > 50)
        LM.landmarks_build_views(ctx, cs["K"], t_dev, s_dev, None, LM.TRI_FIRST_TWO, 0.0)
        got = ctx.landmarks_fetch()
        for k in chained:
            assert got[k].tobytes() == chained[k].tobytes(), (name, k)
        # the other modes read the same poses on the device: equal to the host route with the fetched blocks
        poses6 = VO.window_poses_fetch(ctx)["poses6"]
        for mode in (LM.TRI_WIDEST, LM.TRI_ALL_VIEWS):
            LM.landmarks_build_views(ctx, cs["K"], t_dev, s_dev, None, mode, 3.0)
            dev = (ctx.landmarks_fetch(),) + LM.landmarks_views_fetch(ctx)
            LM.landmarks_build_views(ctx, cs["K"], t_dev, s_dev, poses6, mode, 3.0)
            assert_views_equal(dev, (ctx.landmarks_fetch(),) + LM.landmarks_views_fetch(ctx))


# ---- 2. bit identity with the sequential restatement ----------------------------------------------------------------
@pytest.mark.parametrize("slots,W", SHAPES)
def test_mixed_batch_in_order_and_reversed(pkg, ctx, seq, slots, W):
    scenes = mixed_scenes(slots, W)
    for mode in VS.MODES:
        for gate in GATES:
            ref = VS.seq_views_build(seq, K, *R.stack(scenes), mode, gate)
            # conditions on the reference: what the batch is there to hold
            rank10 = mode == VS.FIRST_TWO and gate == 0.0
            bad_status = R.OK if rank10 and W >= 3 else R.BAD_POSE
            assert list(ref[0]["status"][1:4]) == [R.BASELINE, R.EMPTY, bad_status], (mode, gate)
            assert set(ref[1][2]) <= {VS.BEHIND, VS.SHORT} and np.all(ref[1][1] == VS.NO_WINDOW)
            if slots >= 63:
                assert ref[0]["status"][0] == ref[0]["status"][4] == R.OK
                assert {VS.KEPT, VS.SHORT} <= set(ref[1][0]) and (gate == 0.0 or W < 3 or VS.REPROJECTION in ref[1][4])
            assert_views_equal(gpu_views(pkg, ctx, scenes, mode, gate), ref)
            rev = VS.seq_views_build(seq, K, *R.stack(scenes[::-1]), mode, gate)
            assert_views_equal(gpu_views(pkg, ctx, scenes[::-1], mode, gate), rev)
    v = pkg.orbx_lm.landmarks_views_view(ctx)
    assert (v.n_windows, v.slot_capacity) == (5, slots) and v.reason and v.reproj_px
    # a range of the diagnostics
    reason, px = pkg.orbx_lm.landmarks_views_fetch(ctx, 3, 2)
    assert np.array_equal(reason, rev[1][3:]) and np.array_equal(px.view(np.uint32), rev[2][3:].view(np.uint32))


def test_two_observations_give_one_point_in_every_mode(pkg, ctx):
    sc = R.make_scene(51, W=5, slots=257, sigma=0.3)
    two = np.flatnonzero(sc["seen"] == 2)
    assert len(two) > 30
    points = []
    for mode in VS.MODES:
        block, reason, _ = gpu_views(pkg, ctx, [sc], mode, 0.0)
        assert np.all(reason[0][two] == VS.KEPT)
        points.append(block["points3"][np.searchsorted(block["slot_of_point"], two)])
    assert np.array_equal(u64(points[0]), u64(points[1])) and np.array_equal(u64(points[0]), u64(points[2]))
    block3, _, _ = gpu_views(pkg, ctx, [sc], VS.ALL_VIEWS, 0.0)
    more = np.flatnonzero(sc["seen"] > 2)
    first = gpu_views(pkg, ctx, [sc], VS.FIRST_TWO, 0.0)[0]
    a = block3["points3"][np.searchsorted(block3["slot_of_point"], more)]
    b = first["points3"][np.searchsorted(first["slot_of_point"], more)]
    assert (u64(a) != u64(b)).any(axis=1).all()  # (and with more views the point does move)


def test_offsets_scan_over_several_chunks(pkg, ctx, seq):
    """300 windows of 3-20 live slots: the scan of k_lm_offsets runs over two chunks behind the new kernels"""
    rng = np.random.default_rng(5)
    scenes = []
    for w in range(300):
        sc = R.make_scene(1000 + w, W=3, slots=20, min_seen=1, sigma=0.3, outliers=0.2)
        sc["seen"][int(rng.integers(3, 21)):] = 0
        if w % 97 == 5:
            sc["poses"][1, 3:] = sc["poses"][0, 3:]  # no baseline
        scenes.append(sc)
    ref = VS.seq_views_build(seq, K, *R.stack(scenes), VS.ALL_VIEWS, 3.0)
    assert (ref[0]["status"] == R.BASELINE).sum() == 4 and (ref[0]["status"] == R.OK).sum() > 280
    assert (ref[1] == VS.REPROJECTION).sum() > 100
    assert_views_equal(gpu_views(pkg, ctx, scenes, VS.ALL_VIEWS, 3.0), ref)


# ---- 3. downstream --------------------------------------------------------------------------------------------------
def test_solve_and_write_back_on_an_all_views_block(pkg, ctx):
    scenes = mixed_scenes(257, 5)
    block, reason, _ = gpu_views(pkg, ctx, scenes, VS.ALL_VIEWS, 3.0)
    assert (reason[0] == VS.REPROJECTION).sum() > 10
    _, sums = check_solve(pkg, ctx, scenes, block=block)
    term = [s["termination"] for s in sums]
    assert term[1:4] == [pkg.orbx.BA_SKIPPED] * 3 and pkg.orbx.BA_SKIPPED not in (term[0], term[4]), term
    assert sums[0]["iterations"] >= 1 and sums[0]["final_cost"] <= sums[0]["initial_cost"]
    S.assert_blocks_equal(ctx.landmarks_fetch(), block)
    pkg.orbx_vo.bundle_adjust_write_back(ctx)
    poses4x4, updated = pkg.orbx_vo.bundle_adjust_write_back_fetch(ctx)
    assert poses4x4.shape == (5, 5, 4, 4) and np.isfinite(poses4x4).all() and not updated[1:4].any()
    assert all(term[w] == pkg.orbx.BA_CONVERGENCE for w in range(5) if updated[w].any())


def test_bundle_adjust_tracks_views_is_the_device_pair_on_a_batch_of_one(pkg, ctx, seq):
    LM = pkg.orbx_lm
    scenes = mixed_scenes(257, 5)
    for w, mode, gate in ((0, LM.TRI_ALL_VIEWS, 3.0), (4, LM.TRI_WIDEST, 0.0), (2, LM.TRI_ALL_VIEWS, 3.0)):
        sc = scenes[w]
        block, _, _ = gpu_views(pkg, ctx, [sc], mode, gate)
        ctx.bundle_adjust_landmarks()
        poses, sums, pts = ctx.bundle_adjust_landmarks_fetch()
        hp, hs, st, hx, hslot = LM.bundle_adjust_tracks_views(ctx, K, sc["tracks"], sc["seen"], sc["poses"], mode, gate)
        assert st == block["status"][0] and hs == sums[0]
        assert np.array_equal(u64(hp), u64(poses[0])) and np.array_equal(u64(hx), u64(pts))
        assert np.array_equal(hslot, block["slot_of_point"])
        # the diagnostics are those of the batch of one
        assert_views_equal((ctx.landmarks_fetch(),) + LM.landmarks_views_fetch(ctx),
                           VS.seq_views_build(seq, K, *R.stack([sc]), mode, gate))


# ---- 4. state -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_block_and_diagnostics(pkg, ctx, seq):
    LM, E = pkg.orbx_lm, pkg.orbx
    scenes = mixed_scenes(63, 5)
    poses, tracks, seen = R.stack(scenes)
    d_tracks, d_seen = upload(tracks, seen)
    ref = VS.seq_views_build(seq, K, poses, tracks, seen, VS.ALL_VIEWS, 3.0)
    LM.landmarks_build_views(ctx, K, d_tracks, d_seen, poses, LM.TRI_ALL_VIEWS, 3.0)
    # a window-poses block of another shape (cap5 of the tracks-pose cases: two windows of three frames)
    cs = CASES["cap5"]
    assert (len(cs["seen"]), cs["L"]) != (5, 5)
    ctx.tracks_pose(cs["K"], *upload(cs["tracks"], cs["seen"]), **cs["kw"])
    pkg.orbx_vo.window_poses(ctx)
    nan_K, inf_pose = K.copy(), poses.copy()
    nan_K[1, 1] = np.nan
    inf_pose[3, 2, 4] = np.inf
    bad = [
        (dict(tri_mode=-1), E.ERR_INVALID_ARG), (dict(tri_mode=3), E.ERR_INVALID_ARG),
        (dict(max_reproj_px=-1.0), E.ERR_INVALID_ARG), (dict(max_reproj_px=float("nan")), E.ERR_INVALID_ARG),
        (dict(max_reproj_px=float("inf")), E.ERR_INVALID_ARG),
        (dict(poses=None), E.ERR_INVALID_ARG),  # the window-poses block has another shape
        (dict(K=nan_K), E.ERR_INVALID_ARG), (dict(poses=inf_pose), E.ERR_INVALID_ARG),
        (dict(window_len=9, poses=np.zeros((5, 9, 6))), E.ERR_INVALID_ARG),
        (dict(slot_capacity=0), E.ERR_INVALID_ARG), (dict(tracks=0), E.ERR_INVALID_ARG),
        (dict(slot_capacity=65537), E.ERR_UNSUPPORTED),
    ]
    for kw, status in bad:
        a = dict(tracks=d_tracks.data_ptr(), seen=d_seen.data_ptr(), n_windows=5, slot_capacity=63, window_len=5, K=K,
                 poses=poses, tri_mode=LM.TRI_ALL_VIEWS, max_reproj_px=3.0)
        a.update(kw)
        with pytest.raises(pkg.OrbxError) as e:
            LM.landmarks_build_views(ctx, a.pop("K"), a.pop("tracks"), a.pop("seen"), a.pop("poses"), **a)
        assert e.value.status == status, kw
        assert_views_equal((ctx.landmarks_fetch(),) + LM.landmarks_views_fetch(ctx), ref)
    for first, n in ((5, 1), (-1, 2), (3, 3), (0, 0)):
        with pytest.raises(pkg.OrbxError):
            LM.landmarks_views_fetch(ctx, first, n)
    for kw in (dict(tri_mode=7), dict(max_reproj_px=-0.5)):
        with pytest.raises(pkg.OrbxError) as e:
            LM.bundle_adjust_tracks_views(ctx, K, tracks[0], seen[0], poses[0], **kw)
        assert e.value.status == E.ERR_INVALID_ARG, kw
    assert_views_equal((ctx.landmarks_fetch(),) + LM.landmarks_views_fetch(ctx), ref)
    # a plain build replaces the block and ends the diagnostics
    ctx.landmarks_build(K, d_tracks, d_seen, poses)
    for call in (LM.landmarks_views_view, LM.landmarks_views_fetch):
        with pytest.raises(pkg.OrbxError) as e:
            call(ctx)
        assert e.value.status == E.ERR_INVALID_ARG


def test_null_poses_without_a_window_poses_block_and_views_before_any_build(pkg):
    LM = pkg.orbx_lm
    sc = R.make_scene(1, W=3, slots=5, min_seen=2)
    with pkg.Context(pkg.default_params("gpu", max_width=64, max_height=64, max_batch=2)) as c:
        for call in (LM.landmarks_views_view, LM.landmarks_views_fetch):
            with pytest.raises(pkg.OrbxError) as e:
                call(c)
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        with pytest.raises(pkg.OrbxError) as e:
            LM.landmarks_build_views(c, K, sc["tracks"][None], sc["seen"][None], None)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        with pytest.raises(pkg.OrbxError):
            c.landmarks_fetch()


@pytest.fixture(scope="module")
def rolled():
    """7 frames: the 320 x 160 crop of kitti_000000 rolled by (3, 1) pixels per frame; poses that make such a shift a
    plane at depth 50"""
    crop = np.ascontiguousarray(O.load_kitti(0)[100:260, 300:620])
    frames = np.stack([np.roll(crop, (k, 3 * k), axis=(0, 1)) for k in range(7)])
    poses = np.zeros((3, 5, 6))
    for w in range(3):
        for k in range(5):
            poses[w, k, 3:] = (0.5 * k, k / 6.0, 0.0)
    return frames, poses


def test_build_on_another_stream_than_the_tracker(pkg, ctx, seq, rolled):
    import torch

    LM = pkg.orbx_lm
    frames, poses = rolled
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    hip = pkg.orbx.load()
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
    ctx.good_features_batch(t, 400, 0.01, 8.0, stream=s1.value)
    g = ctx.good_features_view()
    ctx.lk_track_windows(t, [0, 1, 2], 5, g.corners_xy, g.counts, slot_capacity=g.slot_capacity, stream=s1.value)
    LM.landmarks_build_views(ctx, K_CROP, ctx.lk_windows_view(), None, poses, LM.TRI_ALL_VIEWS, 3.0, stream=s2.value)
    ctx.bundle_adjust_landmarks(stream=s2.value)
    assert hip.hipStreamDestroy(s1) == 0 and hip.hipStreamDestroy(s2) == 0
    got = (ctx.landmarks_fetch(),) + LM.landmarks_views_fetch(ctx)
    tracks, seen, _ = ctx.lk_windows_fetch()
    ref = VS.seq_views_build(seq, K_CROP, poses, tracks, seen, VS.ALL_VIEWS, 3.0)
    assert list(ref[0]["status"]) == [R.OK] * 3 and np.diff(ref[0]["point_offset"]).min() > 50
    assert_views_equal(got, ref)
    assert all(s["termination"] != pkg.orbx.BA_SKIPPED for s in ctx.bundle_adjust_landmarks_fetch()[1])


def test_other_results_are_untouched(pkg, ctx, rolled):
    import torch

    LM, VO = pkg.orbx_lm, pkg.orbx_vo
    frames, _ = rolled
    scenes = mixed_scenes(63, 5)
    t = torch.from_numpy(frames[:3]).cuda()
    torch.cuda.synchronize()
    cap = ctx.plan(320, 160)["out_capacity"]
    cs = CASES["cap63"]
    t_dev, s_dev = upload(cs["tracks"], cs["seen"])

    def snapshot():
        out = [ctx.batch_fetch(0, 3, cap)]
        out += [ctx.batch_match_fetch(pair, cap) for pair in (0, 1)]
        wp = VO.window_poses_fetch(ctx)
        return out, ctx.good_features_fetch(), ctx.lk_windows_fetch(), ctx.tracks_pose_fetch(), wp

    ctx.batch_device(t.data_ptr(), 3, 320, 160)
    ctx.batch_match_consecutive(0.8)
    ctx.good_features_batch(t, 300, 0.01, 8.0)
    g = ctx.good_features_view()
    ctx.lk_track_windows(t, [0], 3, g.corners_xy, g.counts, slot_capacity=g.slot_capacity)
    ctx.tracks_pose(cs["K"], t_dev, s_dev, **cs["kw"])
    VO.window_poses(ctx)
    before = snapshot()
    assert before[0][0]["counts"].min() > 50 and len(before[1][0]) > 50 and (before[2][1] == 3).sum() > 50
    gpu_views(pkg, ctx, scenes, VS.ALL_VIEWS, 3.0)
    LM.landmarks_build_views(ctx, cs["K"], t_dev, s_dev, None, LM.TRI_WIDEST, 3.0)
    ctx.bundle_adjust_landmarks()
    ctx.bundle_adjust_landmarks_fetch()
    LM.bundle_adjust_tracks_views(ctx, K, scenes[0]["tracks"], scenes[0]["seen"], scenes[0]["poses"])
    after = snapshot()
    for k in before[0][0]:
        assert np.array_equal(before[0][0][k], after[0][0][k]), k
    for pair in (1, 2):
        assert all(np.array_equal(x, y) for x, y in zip(before[0][pair], after[0][pair]))
    assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
    for blk in (3, 4):
        assert sorted(before[blk]) == sorted(after[blk])
        for k in before[blk]:
            assert np.asarray(before[blk][k]).tobytes() == np.asarray(after[blk][k]).tobytes(), (blk, k)
