"""Landmarks of tracked windows built on the device and bundle-adjusted there (DESIGN.md §9 rank 10;
orbx_landmarks_build_device, orbx_bundle_adjust_landmarks_device and their companions).  The landmarks block is
compared bit for bit -- status, offsets, points, observations, slot_of_point -- with the sequential restatement
tests/cpp/lm_sequential.cpp; the solve bit for bit with orbx_bundle_adjust_batch on the fetched landmark arrays.
Synthetic tracks are uploaded as tensors: no images but in the plumbing test."""
import ctypes as C

import numpy as np
import pytest

import landmarks_ref as R
import landmarks_seq as S
import oracle_lib as O

pytestmark = pytest.mark.gpu
K = R.K_KITTI
OTHER_WORLD = (R.rodrigues(np.array([0.4, -1.1, 0.7])), np.array([3.0, -7.0, 11.0]))


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("lm_seq_gpu"), "lm_sequential")


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def gpu_build(ctx, scenes, **kw):
    poses, tracks, seen = R.stack(scenes)
    ctx.landmarks_build(K, tracks, seen, poses, **kw)
    return ctx.landmarks_fetch()


def seq_of(seq, scenes):
    return S.seq_build(seq, K, *R.stack(scenes))


@pytest.mark.parametrize("slots", [1, 63, 64, 65, 255, 256, 257, 1025, 2000])
def test_slot_counts_all_kept_and_half_kept(ctx, seq, slots):
    """wave, workgroup and chunk boundaries of the fill scan"""
    scenes = [R.make_scene(100 + slots, W=5, slots=slots, min_seen=2),
              R.make_scene(200 + slots, W=5, slots=slots, min_seen=0, world=R.WORLD_TILTED)]
    ref = seq_of(seq, scenes)
    n0, n1 = np.diff(ref["point_offset"])
    assert n0 == slots and (slots < 63 or 0.3 * slots < n1 < 0.8 * slots), (n0, n1)  # conditions on the reference
    got = gpu_build(ctx, scenes)
    S.assert_blocks_equal(got, ref)
    v = ctx.landmarks_view()
    assert (v.n_windows, v.slot_capacity, v.window_len) == (2, slots, 5)


@pytest.mark.parametrize("W", [2, 5, 8])
def test_window_lengths_with_ragged_seen(ctx, seq, W):
    scenes = [R.make_scene(300 + W, W=W, slots=257, min_seen=0, world=OTHER_WORLD, sigma=0.3)]
    assert set(scenes[0]["seen"]) == set(range(W + 1))
    ref = seq_of(seq, scenes)
    assert ref["status"][0] == R.OK and 50 < ref["point_offset"][1] < 257
    S.assert_blocks_equal(gpu_build(ctx, scenes), ref)


def mixed_scenes(slots=300, W=5):
    ok = R.make_scene(401, W=W, slots=slots, min_seen=0, world=R.WORLD_TILTED, sigma=0.3, outliers=0.1, pose_pert=0.002)
    baseline = R.make_scene(402, W=W, slots=slots, min_seen=2)
    baseline["poses"][1, 3:] = baseline["poses"][0, 3:] + np.array([0.01, 0.0, 0.02])
    empty = R.make_scene(403, W=W, slots=slots, min_seen=2, depth_sign=-1.0)
    bad = R.make_scene(404, W=W, slots=slots, min_seen=2)
    bad["poses"][0, :3] = np.array([0.0, 2e5, 0.0])
    last = R.make_scene(405, W=W, slots=slots, min_seen=2)
    last["seen"][:-1] = 0
    first = R.make_scene(406, W=W, slots=slots, min_seen=2)
    first["seen"][1:] = 1
    full = R.make_scene(407, W=W, slots=slots, min_seen=2, pose_pert=0.002)
    return [ok, baseline, empty, bad, last, first, full]


@pytest.fixture(scope="module")
def mixed(seq):
    scenes = mixed_scenes()
    ref = seq_of(seq, scenes)
    assert list(ref["status"]) == [R.OK, R.BASELINE, R.EMPTY, R.BAD_POSE, R.OK, R.OK, R.OK]
    n = np.diff(ref["point_offset"])
    assert 100 < n[0] < 300 and list(n[1:]) == [0, 0, 0, 1, 1, 300]
    assert ref["slot_of_point"][ref["point_offset"][4]] == 299 and ref["slot_of_point"][ref["point_offset"][5]] == 0
    for a in ref.values():
        a.setflags(write=False)
    return scenes, ref


def test_mixed_batch_reversed_and_each_window_alone(ctx, seq, mixed):
    scenes, ref = mixed
    S.assert_blocks_equal(gpu_build(ctx, scenes), ref)
    S.assert_blocks_equal(gpu_build(ctx, scenes[::-1]), seq_of(seq, scenes[::-1]))
    for w, sc in enumerate(scenes):  # a window's block does not depend on its batch
        got = gpu_build(ctx, [sc])
        assert got["status"][0] == ref["status"][w]
        for a, b in zip(S.window_of(got, 0), S.window_of(ref, w)):
            assert a.shape == b.shape and np.array_equal(a, b)
    # a range of the batch
    gpu_build(ctx, scenes)
    part = ctx.landmarks_fetch(4, 3)
    assert list(part["status"]) == [R.OK] * 3 and list(part["point_offset"]) == [0, 1, 2, 302]
    for k in range(3):
        for a, b in zip(S.window_of(part, k), S.window_of(ref, 4 + k)):
            assert np.array_equal(a, b)


def test_offsets_scan_over_several_chunks(ctx, seq):
    """600 windows of 3-20 live slots: the scan of k_lm_offsets runs over three chunks"""
    rng = np.random.default_rng(5)
    scenes = []
    for w in range(600):
        sc = R.make_scene(1000 + w, W=3, slots=20, min_seen=1)
        sc["seen"][int(rng.integers(3, 21)):] = 0
        if w % 97 == 5:
            sc["poses"][1, 3:] = sc["poses"][0, 3:]  # no baseline
        scenes.append(sc)
    ref = seq_of(seq, scenes)
    assert (ref["status"] == R.BASELINE).sum() == 7 and (ref["status"] == R.OK).sum() > 580
    S.assert_blocks_equal(gpu_build(ctx, scenes), ref)


def host_solve(ctx, block, poses, delta, max_iters):
    """orbx_bundle_adjust_batch on the fetched landmark arrays of the OK windows: {window: (poses, points, summary)}"""
    ok = [w for w in range(len(block["status"])) if block["status"][w] == R.OK]
    wins = []
    for w in ok:
        pts, _, op, oq, xy = S.window_of(block, w)
        wins.append((poses[w], pts, op, oq, xy))
    return dict(zip(ok, ctx.bundle_adjust_batch(K, wins, huber_delta=delta, max_iters=max_iters)))


def check_solve(pkg, ctx, scenes, delta=1.0, max_iters=200, block=None):
    poses_in = R.stack(scenes)[0]
    if block is None:
        block = gpu_build(ctx, scenes)
    ctx.bundle_adjust_landmarks(delta, max_iters)
    poses, sums, pts = ctx.bundle_adjust_landmarks_fetch()
    ref = host_solve(ctx, block, poses_in, delta, max_iters)
    assert len(pts) == block["point_offset"][-1]
    for w in range(len(scenes)):
        p0, p1 = block["point_offset"][w], block["point_offset"][w + 1]
        if w in ref:
            rp, rx, rs = ref[w]
            assert sums[w] == rs, (w, sums[w], rs)
            assert np.array_equal(u64(poses[w]), u64(rp)), w
            assert np.array_equal(u64(pts[p0:p1]), u64(rx)), w
        else:
            assert p0 == p1
            assert sums[w] == dict(termination=pkg.orbx.BA_SKIPPED, iterations=0, successful_steps=0,
                                   initial_cost=0.0, final_cost=0.0), sums[w]
            assert np.array_equal(u64(poses[w]), u64(poses_in[w])), w
    return block, sums


def test_solve_equals_the_host_entry_on_the_fetched_arrays(pkg, ctx, mixed):
    scenes, _ = mixed
    block, sums = check_solve(pkg, ctx, scenes)
    term = [s["termination"] for s in sums]
    assert term[1:4] == [pkg.orbx.BA_SKIPPED] * 3 and term[0] == term[6] == pkg.orbx.BA_CONVERGENCE, term
    assert sums[0]["iterations"] >= 2 and sums[6]["iterations"] >= 2  # 0.3 px with 10 % outliers; noiseless
    # the block stays as built: max_iters = 3 (no_convergence), then delta = 2.5, each from the unrefined start
    _, sums3 = check_solve(pkg, ctx, scenes, max_iters=3, block=block)
    assert sums3[0]["termination"] == pkg.orbx.BA_NO_CONVERGENCE and sums3[0]["iterations"] == 3
    _, sums25 = check_solve(pkg, ctx, scenes, delta=2.5, block=block)
    assert sums25[0]["initial_cost"] != sums[0]["initial_cost"]
    S.assert_blocks_equal(ctx.landmarks_fetch(), block)
    # a range of the solve
    poses, s2, pts = ctx.bundle_adjust_landmarks_fetch(4, 3)
    assert len(pts) == 302 and s2 == sums25[4:7]


def test_solve_more_windows_than_workgroups(pkg, ctx):
    """520 OK windows among 530: more than the 512 workgroups of a launch"""
    scenes = [R.make_scene(2000 + w, W=3, slots=12, min_seen=2, sigma=0.3, pose_pert=0.002) for w in range(530)]
    for w in range(0, 530, 53):
        scenes[w]["poses"][1, 3:] = scenes[w]["poses"][0, 3:]
    block, sums = check_solve(pkg, ctx, scenes)
    assert (block["status"] == R.OK).sum() == 520
    assert sum(s["termination"] == pkg.orbx.BA_SKIPPED for s in sums) == 10


def test_bundle_adjust_tracks_is_the_device_pair_on_a_batch_of_one(pkg, ctx, mixed):
    scenes, ref = mixed
    for w in (0, 2, 6):
        sc = scenes[w]
        gpu_build(ctx, [sc])
        ctx.bundle_adjust_landmarks()
        poses, sums, pts = ctx.bundle_adjust_landmarks_fetch()
        hp, hs, st, hx, hslot = ctx.bundle_adjust_tracks(K, sc["tracks"], sc["seen"], sc["poses"])
        assert st == ref["status"][w] and hs == sums[0]
        assert np.array_equal(u64(hp), u64(poses[0])) and np.array_equal(u64(hx), u64(pts))
        assert np.array_equal(hslot, S.window_of(ref, w)[1])


# ---- plumbing: corners -> tracks -> landmarks -> solve without a fetch in between ------------------------------------
K_CROP = np.array([[300.0, 0.0, 160.0], [0.0, 300.0, 80.0], [0.0, 0.0, 1.0]])


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


def test_device_chain_equals_the_fetched_and_reuploaded_chain(pkg, ctx, rolled):
    import torch

    frames, poses = rolled
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    hip = pkg.orbx.load()
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    ctx.good_features_batch(t, 400, 0.01, 8.0, stream=s.value)
    g = ctx.good_features_view()
    ctx.lk_track_windows(t, [0, 1, 2], 5, g.corners_xy, g.counts, slot_capacity=g.slot_capacity, stream=s.value)
    v = ctx.lk_windows_view()
    ctx.landmarks_build(K_CROP, v.tracks_xy, v.seen, poses, n_windows=3, slot_capacity=v.slot_capacity, window_len=5,
                        stream=s.value)
    ctx.bundle_adjust_landmarks(stream=s.value)
    assert hip.hipStreamDestroy(s) == 0
    dev_block = ctx.landmarks_fetch()
    dev_solve = ctx.bundle_adjust_landmarks_fetch()
    assert list(dev_block["status"]) == [R.OK] * 3 and np.diff(dev_block["point_offset"]).min() > 50
    # the host route: every stage fetched and uploaded again
    corners = ctx.good_features_fetch()
    cap = g.slot_capacity
    pts = np.zeros((3, cap, 2), np.float32)
    for w in range(3):
        pts[w, :len(corners[w])] = corners[w]
    ctx.lk_track_windows(frames, [0, 1, 2], 5, pts, np.int32([len(corners[w]) for w in range(3)]))
    tracks, seen, _ = ctx.lk_windows_fetch()
    ctx.landmarks_build(K_CROP, tracks, seen, poses)
    host_block = ctx.landmarks_fetch()
    S.assert_blocks_equal(host_block, dev_block)
    wins = [(poses[w],) + tuple(S.window_of(host_block, w)[i] for i in (0, 2, 3, 4)) for w in range(3)]
    host = ctx.bundle_adjust_batch(K_CROP, wins)
    for w in range(3):
        p0, p1 = host_block["point_offset"][w], host_block["point_offset"][w + 1]
        assert dev_solve[1][w] == host[w][2]
        assert np.array_equal(u64(dev_solve[0][w]), u64(host[w][0]))
        assert np.array_equal(u64(dev_solve[2][p0:p1]), u64(host[w][1]))


def test_other_results_are_untouched(ctx, rolled, mixed):
    import torch

    frames, _ = rolled
    scenes, ref = mixed
    t = torch.from_numpy(frames[:3]).cuda()
    torch.cuda.synchronize()
    cap = ctx.plan(320, 160)["out_capacity"]
    ba_win = S.window_of(ref, 0)
    ba_args = (K, scenes[0]["poses"], ba_win[0], ba_win[2], ba_win[3], ba_win[4])

    def snapshot():
        out = [ctx.batch_fetch(0, 3, cap)]
        out += [ctx.batch_match_fetch(pair, cap) for pair in (0, 1)]
        return out, ctx.good_features_fetch(), ctx.lk_windows_fetch(), ctx.bundle_adjust(*ba_args)

    ctx.batch_device(t.data_ptr(), 3, 320, 160)
    ctx.batch_match_consecutive(0.8)
    ctx.good_features_batch(t, 300, 0.01, 8.0)
    g = ctx.good_features_view()
    ctx.lk_track_windows(t, [0], 3, g.corners_xy, g.counts, slot_capacity=g.slot_capacity)
    before = snapshot()
    assert before[0][0]["counts"].min() > 50 and len(before[1][0]) > 50 and (before[2][1] == 3).sum() > 50
    S.assert_blocks_equal(gpu_build(ctx, scenes), ref)
    ctx.bundle_adjust_landmarks()
    ctx.bundle_adjust_landmarks_fetch()
    ctx.bundle_adjust_tracks(K, scenes[6]["tracks"], scenes[6]["seen"], scenes[6]["poses"])
    after = snapshot()
    for k in before[0][0]:
        assert np.array_equal(before[0][0][k], after[0][0][k]), k
    for pair in (1, 2):
        assert all(np.array_equal(x, y) for x, y in zip(before[0][pair], after[0][pair]))
    assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
    assert np.array_equal(u64(before[3][0]), u64(after[3][0])) and np.array_equal(u64(before[3][1]), u64(after[3][1]))
    assert before[3][2] == after[3][2]


def test_refusals_leave_the_previous_block(pkg, ctx, mixed):
    import torch

    scenes, ref = mixed
    poses, tracks, seen = R.stack(scenes)
    d_tracks, d_seen = torch.from_numpy(tracks).cuda(), torch.from_numpy(seen).cuda()
    torch.cuda.synchronize()
    ctx.landmarks_build(K, d_tracks, d_seen, poses)
    E = pkg.orbx
    nan_K, inf_pose = K.copy(), poses.copy()
    nan_K[1, 1] = np.nan
    inf_pose[3, 2, 4] = np.inf
    raw = dict(tracks=d_tracks.data_ptr(), seen=d_seen.data_ptr(), n_windows=7, slot_capacity=300, window_len=5)
    bad = [
        (dict(window_len=1, poses=poses[:, :1]), E.ERR_INVALID_ARG),
        (dict(window_len=9, poses=np.zeros((7, 9, 6))), E.ERR_INVALID_ARG),
        (dict(n_windows=0, poses=np.zeros((0, 5, 6))), E.ERR_INVALID_ARG),
        (dict(slot_capacity=0), E.ERR_INVALID_ARG),
        (dict(tracks=0), E.ERR_INVALID_ARG),
        (dict(seen=0), E.ERR_INVALID_ARG),
        (dict(K=nan_K), E.ERR_INVALID_ARG),
        (dict(poses=inf_pose), E.ERR_INVALID_ARG),
        (dict(slot_capacity=65537), E.ERR_UNSUPPORTED),
        (dict(n_windows=40000, slot_capacity=60000, window_len=2, poses=np.zeros((40000, 2, 6))), E.ERR_UNSUPPORTED),
        (dict(n_windows=300000, slot_capacity=2000, window_len=5, poses=np.zeros((300000, 5, 6))), E.ERR_UNSUPPORTED),
    ]
    for kw, status in bad:
        a = dict(raw, K=K, poses=poses)
        a.update(kw)
        with pytest.raises(pkg.OrbxError) as e:
            ctx.landmarks_build(a.pop("K"), a.pop("tracks"), a.pop("seen"), a.pop("poses"), **a)
        assert e.value.status == status, kw
        S.assert_blocks_equal(ctx.landmarks_fetch(), ref)
    for kw in (dict(huber_delta=0.0), dict(huber_delta=float("nan")), dict(max_iters=0), dict(max_iters=1001)):
        with pytest.raises(pkg.OrbxError) as e:
            ctx.bundle_adjust_landmarks(**kw)
        assert e.value.status == E.ERR_INVALID_ARG, kw
    for first, n in ((7, 1), (-1, 2), (5, 3), (0, 0)):
        with pytest.raises(pkg.OrbxError):
            ctx.landmarks_fetch(first, n)
    with pytest.raises(pkg.OrbxError):  # built, not solved since
        ctx.bundle_adjust_landmarks_fetch()
    # the capacity convention: the required counts, nothing else written
    f = pkg.orbx.load().orbx_landmarks_fetch
    npt, nob, pts = C.c_int(0), C.c_int(0), np.full((10, 3), 7.0)
    st = f(ctx._h, 0, 7, None, None, None, None, pts.ctypes.data_as(C.c_void_p), None, 10, None, None, None, 0,
           C.byref(npt), C.byref(nob))
    assert st == E.ERR_CAPACITY and npt.value == ref["point_offset"][7] and nob.value == ref["obs_offset"][7]
    assert (pts == 7.0).all()
    S.assert_blocks_equal(ctx.landmarks_fetch(), ref)


def test_solve_and_views_before_any_build_are_refused(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=64, max_height=64, max_batch=2)) as c:
        for call in (c.landmarks_view, c.landmarks_fetch, c.bundle_adjust_landmarks, c.bundle_adjust_landmarks_fetch):
            with pytest.raises(pkg.OrbxError) as e:
                call()
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
