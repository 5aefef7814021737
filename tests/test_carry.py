"""Landmarks carried into the next generation of windows and those windows localised by PnP on the device (DESIGN.md §9
rank 18; include/orbx_carry.h).  The carry block, the records, poses6, masks and window_status are compared byte for
byte with tests/carry_ref.py run on the FETCHED landmarks block (whose own parity tests/test_landmarks.py pins): the
join and the gather in numpy, each problem's solve by tests/cpp/pnp_sequential.cpp.  Synthetic tracks are uploaded as
arrays: no images.

The bounds of test_the_scale_stays, measured on the CPU from the reference alone (carry_ref + pnp_seq + landmarks_seq;
tests/test_carry_ref.py repeats the measurement without a GPU): over generations 1 and 2 of two streams whose first map
is 3 x too large, every pair's |relative translation| deviates from 3 x the true one by at most SCALE_RATIO_MEASURED
(relative), its rotation from the true one by at most SCALE_ROT_MEASURED rad, and frame 0 of every window lies at most
FRAME0_ROT_MEASURED rad and FRAME0_T_MEASURED map units from the previous window's true last pose -> ten times that on
the device path (the device is bit-identical to the reference; the margin covers the landmarks build's own parity)."""
import numpy as np
import pytest

import carry_ref as R
import landmarks_ref as L
import landmarks_seq as LS
import pnp_seq as S

pytestmark = pytest.mark.gpu
K = R.K
PARAMS = R.MIX_PARAMS
SCALE_RATIO_MEASURED, SCALE_ROT_MEASURED = 8.0e-7, 2.3e-8    # measured: 7.98e-7, 2.21e-8 rad
FRAME0_ROT_MEASURED, FRAME0_T_MEASURED = 5.0e-8, 4.5e-6      # measured: 4.95e-8 rad, 4.42e-6 units


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("pnp_seq_carry_gpu"))


@pytest.fixture(scope="module")
def mixed():
    return R.mixed_batch()


def build_old(ctx, olds, **kw):
    poses, tracks, seen = R.stack_old(olds)
    ctx.landmarks_build(K, tracks, seen, poses, **kw)


def carry_and_localise(pkg, ctx, news, source=R.CARRY_BUILT, **params):
    origin, tracks, seen = R.stack_new(news)
    pkg.orbx_carry.landmarks_carry(ctx, origin, source=source)
    pkg.orbx_carry.window_poses_pnp_carried(ctx, K, tracks, seen, **params)
    return pkg.orbx_carry.landmarks_carry_fetch(ctx), pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx)


def reference(seq, block, news, cap, points=None, **params):
    origin, tracks, seen = R.stack_new(news)
    carry = R.join(block, origin, cap, points)
    return carry, R.localise(seq, carry, tracks, seen, **params)


def assert_carry_equal(got, ref):
    for k, dt in (("xyz", np.float64), ("point", np.int32), ("count", np.int32)):
        assert got[k].dtype == dt and got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), k


def assert_equal(got, ref):
    """records, poses6, masks and window_status, byte for byte"""
    assert got["records"].dtype == S.RECORD and got["records"].shape == ref["records"].shape
    for name in S.RECORD.names:
        assert got["records"][name].tobytes() == ref["records"][name].tobytes(), name
    assert got["records"].tobytes() == ref["records"].tobytes()
    assert got["poses6"].tobytes() == ref["poses6"].tobytes()
    assert got["window_status"].dtype == np.int32 and got["window_status"].tobytes() == ref["window_status"].tobytes()
    assert got["mask"].shape == ref["mask"].shape and got["mask"].tobytes() == ref["mask"].tobytes()


def test_bit_parity_on_the_mixed_batch(pkg, ctx, seq, mixed):
    olds, news = mixed
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    got_carry, got = carry_and_localise(pkg, ctx, news, **PARAMS)
    carry, ref = reference(seq, block, news, R.MIX_CAP, **PARAMS)
    R.check_mixed(block, carry, ref, news)  # every window is what it is there for
    assert_carry_equal(got_carry, carry)
    assert_equal(got, ref)
    # the views, a range of the batch, one mask
    v = pkg.orbx_carry.landmarks_carry_view(ctx)
    assert (v.n_windows, v.slot_capacity) == (8, R.MIX_CAP) and v.xyz and v.point and v.count
    v = pkg.orbx_carry.window_poses_pnp_carried_view(ctx)
    assert (v.n_windows, v.window_len, v.slot_capacity) == (8, R.MIX_W, R.MIX_CAP)
    part = pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx, 3, 4, masks=False)
    assert part["records"].tobytes() == ref["records"][3:7].tobytes()
    assert part["poses6"].tobytes() == ref["poses6"][3:7].tobytes()
    assert part["window_status"].tolist() == ref["window_status"][3:7].tolist()
    assert pkg.orbx_carry.landmarks_carry_fetch(ctx, 2, 1)["point"].tobytes() == carry["point"][2:3].tobytes()
    with pytest.raises(pkg.OrbxError):
        pkg.orbx_carry.window_poses_pnp_carried_mask(ctx, 0, R.MIX_W)  # k outside [0, window_len)
    with pytest.raises(pkg.OrbxError):
        pkg.orbx_carry.window_poses_pnp_carried_mask(ctx, 0, 0, capacity=R.MIX_CAP - 1)
    # the old block is as it was; the carried build makes the LOST windows BAD_POSE, with no landmark
    LS.assert_blocks_equal(ctx.landmarks_fetch(), block)
    _, tracks, seen = R.stack_new(news)
    pkg.orbx_carry.landmarks_build_carried(ctx, K, tracks, seen)
    new_block = ctx.landmarks_fetch()
    assert list(new_block["status"]) == [L.OK, L.OK, L.OK, L.BAD_POSE, L.BAD_POSE, L.OK, L.OK, L.OK]
    for w in (3, 4):
        assert new_block["point_offset"][w] == new_block["point_offset"][w + 1]
    # the carry block survives the build
    assert_carry_equal(pkg.orbx_carry.landmarks_carry_fetch(ctx), carry)


@pytest.mark.parametrize("change", [dict(max_iters=0), dict(refine_iters=0), dict(refine_iters=20, min_inliers=30)])
def test_bit_parity_with_other_parameters(pkg, ctx, seq, mixed, change):
    olds, news = [m[1:5] for m in mixed]
    params = dict(PARAMS, **change)
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    got_carry, got = carry_and_localise(pkg, ctx, news, **params)
    carry, ref = reference(seq, block, news, R.MIX_CAP, **params)
    assert_carry_equal(got_carry, carry)
    assert_equal(got, ref)
    if params["max_iters"] == 0:
        assert (ref["records"]["status"][:2] == S.NO_MODEL).all() and (ref["window_status"] == R.CARRY_LOST).all()
    else:
        assert (ref["records"]["status"][:2] == S.OK).all()


def test_sources(pkg, ctx, seq, mixed):
    olds, news = [m[:3] for m in mixed]
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    origin, tracks, seen = R.stack_new(news)
    with pytest.raises(pkg.OrbxError):  # the block has not been solved
        pkg.orbx_carry.landmarks_carry(ctx, origin, source=R.CARRY_SOLVED)
    with pytest.raises(pkg.OrbxError):
        pkg.orbx_carry.landmarks_carry(ctx, origin, source=2)
    ctx.bundle_adjust_landmarks()
    _, summaries, solved = ctx.bundle_adjust_landmarks_fetch()
    assert solved.tobytes() != block["points3"].tobytes()  # the solve moved the points (float32 pixels)
    got_carry, got = carry_and_localise(pkg, ctx, news, source=R.CARRY_SOLVED, **PARAMS)
    carry, ref = reference(seq, block, news, R.MIX_CAP, points=solved, **PARAMS)
    assert_carry_equal(got_carry, carry)
    assert_equal(got, ref)
    p0 = block["point_offset"][1]
    assert got_carry["xyz"][1, 0].tobytes() == solved[p0 + got_carry["point"][1, 0]].tobytes()
    # BUILT behind a solve still carries the block's points
    got_carry, _ = carry_and_localise(pkg, ctx, news, source=R.CARRY_BUILT, **PARAMS)
    assert_carry_equal(got_carry, R.join(block, origin, R.MIX_CAP))
    assert got_carry["xyz"][1, 0].tobytes() == block["points3"][p0 + got_carry["point"][1, 0]].tobytes()


def test_frames_2_and_later_equal_rank_17(pkg, ctx):
    """the identity origin and the old tracks: the same rules and the same seeds give the same bytes"""
    W, cap = 5, 65
    scenes = [L.make_scene(700 + w, W=W, slots=cap, min_seen=W if w < 2 else 2) for w in range(4)]
    poses, tracks, seen = L.stack(scenes)
    ctx.landmarks_build(K, tracks, seen, poses)
    block = ctx.landmarks_fetch()
    pkg.orbx_pnp.window_poses_pnp(ctx, **PARAMS)
    r17 = pkg.orbx_pnp.window_poses_pnp_fetch(ctx)
    assert (r17["records"]["status"] == S.OK).all()
    origin = np.tile(np.arange(cap, dtype=np.int32), (4, 1))
    pkg.orbx_carry.landmarks_carry(ctx, origin)
    pkg.orbx_carry.window_poses_pnp_carried(ctx, K, tracks, seen, **PARAMS)
    got = pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx)
    carry = pkg.orbx_carry.landmarks_carry_fetch(ctx)
    assert got["records"][:, 2:].tobytes() == r17["records"].tobytes()
    assert (got["records"]["n_corr"][2:, 2] < got["records"]["n_corr"][2:, 1]).all()  # seen thins the later frames
    for w in range(4):
        p0, p1 = block["point_offset"][w], block["point_offset"][w + 1]
        slots = block["slot_of_point"][p0:p1]
        assert carry["count"][w] == p1 - p0 and np.array_equal(np.flatnonzero(carry["point"][w] >= 0), slots)
        for k in range(2, W):
            assert got["mask"][w, k, slots].tobytes() == r17["masks"][w][k - 2].tobytes(), (w, k)
            assert got["mask"][w, k].sum() == r17["masks"][w][k - 2].sum()
    # rank 17's block is still there
    assert pkg.orbx_pnp.window_poses_pnp_fetch(ctx, masks=False)["records"].tobytes() == r17["records"].tobytes()


def test_batch_independence(pkg, ctx, seq):
    """70 windows of 5 frames of 8 slots: 350 workgroups, tiny problems; window 37 gives the same bytes alone"""
    W = 5
    pairs = [R.two_generations(400 + w, W, 8, 0, min_seen=4, cap=8)[1:] for w in range(70)]
    olds = [dict(o, poses=o["true_poses"]) for o, _ in pairs]
    news = [n for _, n in pairs]
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    got_carry, got = carry_and_localise(pkg, ctx, news, **PARAMS)
    carry, ref = reference(seq, block, news, 8, **PARAMS)
    assert_carry_equal(got_carry, carry)
    assert_equal(got, ref)
    st = ref["records"]["status"]
    assert (st == S.OK).sum() > 100 and (st == S.FEW_POINTS).sum() > 40 and ref["window_status"][37] == R.CARRY_OK
    build_old(ctx, olds[37:38])
    alone_carry, alone = carry_and_localise(pkg, ctx, news[37:38], **PARAMS)
    assert alone_carry["xyz"].tobytes() == got_carry["xyz"][37:38].tobytes()
    assert alone["records"].tobytes() == got["records"][37:38].tobytes()
    assert alone["poses6"].tobytes() == got["poses6"][37:38].tobytes()
    assert alone["mask"].tobytes() == got["mask"][37:38].tobytes()


def test_the_scale_stays(pkg, ctx):
    """three generations of two streams; generation 0 is built 3 x too large and no solve runs"""
    wins = R.scale_streams()
    stack = lambda g, key: np.stack([w[key] for w in wins[g]])
    ctx.landmarks_build(K, stack(0, "tracks"), stack(0, "seen"), np.stack([R.scaled(w["true_poses"], 3.0) for w in wins[0]]))
    results = []
    for g in (1, 2):
        pkg.orbx_carry.landmarks_carry(ctx, stack(g, "origin"))
        pkg.orbx_carry.window_poses_pnp_carried(ctx, K, stack(g, "tracks"), stack(g, "seen"), **PARAMS)
        pkg.orbx_carry.landmarks_build_carried(ctx, K, stack(g, "tracks"), stack(g, "seen"))
        results.append(pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx))
        assert (ctx.landmarks_fetch()["status"] == L.OK).all()
    ratio, rot, rot0, t0 = R.scale_deviation(results, wins, 3.0)
    print("device: ratio %.3e, rotation %.3e rad, frame 0: %.3e rad, %.3e units" % (ratio, rot, rot0, t0))
    assert ratio <= 10 * SCALE_RATIO_MEASURED and rot <= 10 * SCALE_ROT_MEASURED
    assert rot0 <= 10 * FRAME0_ROT_MEASURED and t0 <= 10 * FRAME0_T_MEASURED


def host_solve(ctx, block, poses, delta=1.0, max_iters=200):
    ok = [w for w in range(len(block["status"])) if block["status"][w] == L.OK]
    wins = []
    for w in ok:
        pts, _, op, oq, xy = LS.window_of(block, w)
        wins.append((poses[w], pts, op, oq, xy))
    return dict(zip(ok, ctx.bundle_adjust_batch(K, wins, huber_delta=delta, max_iters=max_iters)))


def test_build_and_solve_behind_it(pkg, ctx, mixed):
    pick = [0, 1, 2, 6, 7]  # (a LOST window's zeros are BASELINE to the build from host poses, BAD_POSE to the carried)
    olds, news = [[m[w] for w in pick] for m in mixed]
    build_old(ctx, olds)
    _, got = carry_and_localise(pkg, ctx, news, **PARAMS)
    assert (got["window_status"] == R.CARRY_OK).all()
    _, tracks, seen = R.stack_new(news)
    pkg.orbx_carry.landmarks_build_carried(ctx, K, tracks, seen)
    carried = ctx.landmarks_fetch()
    ctx.bundle_adjust_landmarks()
    sp, ss, sx = ctx.bundle_adjust_landmarks_fetch()
    ctx.landmarks_build(K, tracks, seen, got["poses6"])
    LS.assert_blocks_equal(carried, ctx.landmarks_fetch())
    assert (carried["status"] == L.OK).all() and carried["point_offset"][-1] > 400
    ref = host_solve(ctx, carried, got["poses6"])
    for w in range(len(pick)):
        p0, p1 = carried["point_offset"][w], carried["point_offset"][w + 1]
        rp, rx, rs = ref[w]
        assert ss[w] == rs, (w, ss[w], rs)
        assert sp[w].tobytes() == rp.tobytes() and sx[p0:p1].tobytes() == rx.tobytes(), w


def test_refusals_write_nothing(pkg, mixed):
    olds, news = [m[:2] for m in mixed]
    origin, tracks, seen = R.stack_new(news)
    oc = pkg.orbx_carry
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as ctx:
        with pytest.raises(pkg.OrbxError):  # no landmarks block
            oc.landmarks_carry(ctx, origin)
        build_old(ctx, olds)
        with pytest.raises(pkg.OrbxError):  # carried PnP before any carry
            oc.window_poses_pnp_carried(ctx, K, tracks, seen, **PARAMS)
        with pytest.raises(pkg.OrbxError):  # carried build before any carried PnP
            oc.landmarks_build_carried(ctx, K, tracks, seen)
        for fetch in (oc.landmarks_carry_fetch, oc.window_poses_pnp_carried_fetch):
            with pytest.raises(pkg.OrbxError):
                fetch(ctx)
        carry0, got0 = carry_and_localise(pkg, ctx, news, **PARAMS)
        block0 = ctx.landmarks_fetch()
        with pytest.raises(pkg.OrbxError):  # wrong n_windows
            oc.landmarks_carry(ctx, origin[:1])
        with pytest.raises(pkg.OrbxError):  # sizes that differ from the carry block's
            oc.window_poses_pnp_carried(ctx, K, tracks[:1], seen[:1], **PARAMS)
        with pytest.raises(pkg.OrbxError):
            oc.window_poses_pnp_carried(ctx, K, tracks[:, :100], seen[:, :100], **PARAMS)
        for bad in (dict(min_inliers=3), dict(refine_iters=21), dict(threshold_px=float("nan")), dict(max_iters=-1),
                    dict(prob=float("inf"))):
            with pytest.raises(pkg.OrbxError):
                oc.window_poses_pnp_carried(ctx, K, tracks, seen, **dict(PARAMS, **bad))
        long = np.zeros((2, R.MIX_CAP, 9, 2), np.float32)
        with pytest.raises(pkg.OrbxError):  # window_len 9
            oc.window_poses_pnp_carried(ctx, K, long, seen, **PARAMS)
        with pytest.raises(pkg.OrbxError):  # window_len 1
            oc.window_poses_pnp_carried(ctx, K, long[:, :, :1], seen, **PARAMS)
        Kbad = K.copy()
        Kbad[0, 0] = 0.0
        with pytest.raises(pkg.OrbxError):
            oc.window_poses_pnp_carried(ctx, Kbad, tracks, seen, **PARAMS)
        # the previous blocks stay fetchable with the same bytes
        assert_carry_equal(oc.landmarks_carry_fetch(ctx), carry0)
        assert_equal(oc.window_poses_pnp_carried_fetch(ctx), got0)
        # a carried build behind a NEWER carried PnP of other sizes is refused, and the landmarks block stays
        longer = np.concatenate([tracks, tracks[:, :, :1]], axis=2)  # window_len 5
        oc.window_poses_pnp_carried(ctx, K, longer, seen, **PARAMS)
        with pytest.raises(pkg.OrbxError):
            oc.landmarks_build_carried(ctx, K, tracks, seen)
        with pytest.raises(pkg.OrbxError):
            oc.landmarks_build_carried(ctx, K, longer[:1], seen[:1])
        LS.assert_blocks_equal(ctx.landmarks_fetch(), block0)
        assert oc.window_poses_pnp_carried_view(ctx).window_len == 5
        oc.landmarks_build_carried(ctx, K, longer, seen)  # ... and with the PnP's sizes it is taken
        assert ctx.landmarks_view().window_len == 5


def test_callers_streams(pkg, ctx, seq, mixed):
    import torch

    olds, news = [m[:4] for m in mixed]
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    carry, ref = reference(seq, block, news, R.MIX_CAP, **PARAMS)
    build_old(ctx, mixed[0][4:8])  # other blocks in between
    carry_and_localise(pkg, ctx, mixed[1][4:8], **PARAMS)
    origin, tracks, seen = R.stack_new(news)
    d_origin, d_tracks, d_seen = (torch.from_numpy(a).cuda() for a in (origin, tracks, seen))
    torch.cuda.synchronize()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    build_old(ctx, olds, stream=s1.cuda_stream)
    pkg.orbx_carry.landmarks_carry(ctx, d_origin, stream=s2.cuda_stream)  # no synchronisation in between
    pkg.orbx_carry.window_poses_pnp_carried(ctx, K, d_tracks, d_seen, stream=s2.cuda_stream, **PARAMS)
    pkg.orbx_carry.landmarks_build_carried(ctx, K, d_tracks, d_seen, stream=s3.cuda_stream)
    assert_carry_equal(pkg.orbx_carry.landmarks_carry_fetch(ctx), carry)
    got = pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx)
    assert_equal(got, ref)
    on_streams = ctx.landmarks_fetch()
    ctx.landmarks_build(K, tracks[:3], seen[:3], got["poses6"][:3])
    plain = ctx.landmarks_fetch()
    for k in ("points3", "slot_of_point", "obs_xy"):  # windows 0 .. 2 are OK: the same landmarks
        assert on_streams[k][:len(plain[k])].tobytes() == plain[k].tobytes(), k
    assert list(on_streams["status"]) == [L.OK, L.OK, L.OK, L.BAD_POSE]
    torch.cuda.synchronize()


def test_host_entry_drops_landmarks_that_are_not_finite(pkg, ctx, seq, mixed):
    """Rule A's finite test.  Neither source of the batched carry can hold such a coordinate (the build drops the
    landmark, the solve hands its input back when a step fails), so it is reached through the host entry, whose old
    points are the caller's."""
    olds, news = [m[:1] for m in mixed]
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    pts, slots, _, _, _ = LS.window_of(block, 0)
    new = news[0]
    clean = R.join(block, new["origin"][None], R.MIX_CAP)
    bad = pts.copy()
    bad[3, 0], bad[10, 2], bad[20, 1], bad[64] = np.nan, np.inf, -np.inf, (np.nan, np.inf, 0.0)
    carry = R.join(block, new["origin"][None], R.MIX_CAP, points=bad)
    dropped = np.flatnonzero((clean["point"][0] >= 0) & (carry["point"][0] < 0))
    assert sorted(new["origin"][dropped].tolist()) == sorted(slots[[3, 10, 20, 64]].tolist())
    assert not carry["xyz"][0, dropped].any() and np.isfinite(carry["xyz"]).all() and carry["count"][0] == 61
    ref = R.localise(seq, carry, new["tracks"][None], new["seen"][None], **PARAMS)
    assert (ref["records"]["status"] == S.OK).all() and (ref["records"]["n_corr"] == 61).all()
    one = pkg.orbx_carry.localise_carried_window(ctx, bad, slots, new["origin"], new["tracks"], new["seen"], K, **PARAMS)
    assert one["carried_point"].tobytes() == carry["point"][0].tobytes()
    assert one["records"].tobytes() == ref["records"][0].tobytes()
    assert one["poses6"].tobytes() == ref["poses6"][0].tobytes() and one["window_status"] == R.CARRY_OK
    got = pkg.orbx_carry.landmarks_carry_fetch(ctx)  # the entry's own batch of one
    assert got["xyz"].tobytes() == carry["xyz"].tobytes() and got["count"].tobytes() == carry["count"].tobytes()


def test_host_entry(pkg, ctx, seq, mixed):
    olds, news = mixed
    build_old(ctx, olds)
    block = ctx.landmarks_fetch()
    _, batched = carry_and_localise(pkg, ctx, news, **PARAMS)
    carry = pkg.orbx_carry.landmarks_carry_fetch(ctx)
    ctx.bundle_adjust_landmarks()
    solved = ctx.bundle_adjust_landmarks_fetch()
    pkg.orbx_pnp.window_poses_pnp(ctx, **PARAMS)
    r17 = pkg.orbx_pnp.window_poses_pnp_fetch(ctx, masks=False)
    for w in (1, 2, 4, 5, 7):
        pts, slots, _, _, _ = LS.window_of(block, w)
        one = pkg.orbx_carry.localise_carried_window(ctx, pts, slots, news[w]["origin"], news[w]["tracks"],
                                                     news[w]["seen"], K, **PARAMS)
        assert one["records"].tobytes() == batched["records"][w].tobytes(), w
        assert one["poses6"].tobytes() == batched["poses6"][w].tobytes(), w
        assert one["window_status"] == batched["window_status"][w]
        # (window 2's origins beyond the old capacity: the host entry knows no capacity, and no landmark has such a slot)
        assert one["carried_point"].tobytes() == carry["point"][w].tobytes(), w
        # it has replaced the carry and the carried-PnP blocks by its own batch of one
        assert pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx)["records"].tobytes() == one["records"].tobytes()
        assert pkg.orbx_carry.landmarks_carry_fetch(ctx)["point"].tobytes() == one["carried_point"].tobytes()
    # an old window without a landmark: SKIPPED and LOST
    none = pkg.orbx_carry.localise_carried_window(ctx, np.zeros((0, 3)), np.zeros(0, np.int32), news[0]["origin"],
                                                  news[0]["tracks"], news[0]["seen"], K, **PARAMS)
    assert (none["records"]["status"] == S.SKIPPED).all() and none["window_status"] == R.CARRY_LOST
    assert (none["carried_point"] == -1).all() and not none["poses6"].any()
    with pytest.raises(pkg.OrbxError):
        pkg.orbx_carry.localise_carried_window(ctx, np.zeros((0, 3)), np.zeros(0, np.int32), news[0]["origin"],
                                               news[0]["tracks"], news[0]["seen"], K, **dict(PARAMS, min_inliers=3))
    # afterwards the batched blocks of the other calls are still there
    LS.assert_blocks_equal(ctx.landmarks_fetch(), block)
    again = ctx.bundle_adjust_landmarks_fetch()
    assert again[0].tobytes() == solved[0].tobytes() and again[2].tobytes() == solved[2].tobytes()
    assert pkg.orbx_pnp.window_poses_pnp_fetch(ctx, masks=False)["records"].tobytes() == r17["records"].tobytes()
