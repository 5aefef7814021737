"""GPU tests of the window-poses path (include/orbx_vo.h).  The rule throughout: the new route
has to equal the existing route fed with the fetched intermediates, bit for bit.

  chain   orbx_window_poses_device after orbx_tracks_pose_device == tests/cpp/wp_sequential.cpp on what
          orbx_tracks_pose_fetch returns
  build   orbx_landmarks_build_chained_device == orbx_landmarks_build_device with the fetched poses6 from the host,
          and so is the solve behind it
  gate    orbx_bundle_adjust_write_back_device == the sequential gate on the fetched solve, and its `updated` is what
          orbx::detail::ba_write_back (host/orb.hpp) decides
  state   refusals keep the previous block, caller streams, growth, and the other side paths' blocks stay untouched
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import landmarks_ref as LR
import landmarks_seq as LS
import tracks_pose_ref as T
import window_poses_ref as WR
import window_poses_seq as WS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {cs["name"]: cs for cs in T.gpu_cases()}
CHAIN_CASES = ("cap1_L3", "cap5", "cap63", "cap65", "cap257")
I9 = np.eye(3).reshape(9)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return WS.compile_seq(tmp_path_factory.mktemp("wp_seq_gpu"))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wp_mirror_gpu") / "wp_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(pk, "host"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "wp_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def upload(*arrays):
    import torch

    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def first_poses(n, seed):
    """n camera -> world poses (rotations up to 1 rad, translations of a few units) and n scales in [0.1, 5]"""
    rng = np.random.default_rng(seed)
    T0 = np.stack([WR.rigid(WR.rot(rng.normal(size=3), rng.uniform(0.0, 1.0)), rng.normal(size=3) * 3.0)
                   for _ in range(n)])
    return T0, rng.uniform(0.1, 5.0, n)


def posed(c, cs, tracks=None, **kw):
    """tracks pose of a case on the device; returns the device tensors and the fetched R, t, scale per window"""
    t, s = upload(cs["tracks"] if tracks is None else tracks, cs["seen"])
    c.tracks_pose(cs["K"], t, s, **dict(cs["kw"], **kw))
    f = c.tracks_pose_fetch()
    n, L = len(cs["seen"]), cs["L"]
    return (t, s), (f["R"].reshape(n, L - 1, 3, 3), f["t"].reshape(n, L - 1, 3), f["scale"].reshape(n, L - 1))


def assert_chain_equal(got, ref, windows=None):
    for k in ("poses6", "poses4x4", "status"):
        a, b = (got[k], ref[k]) if windows is None else (got[k][windows], ref[k][windows])
        assert WS.bits_equal(a, b), k


# ---- 1. chain -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_chain_equals_the_sequential_restatement(pkg, ctx, seq, name, given):
    VO, cs = pkg.orbx_vo, CASES[name]
    n, L = len(cs["seen"]), cs["L"]
    _, (R, t, scale) = posed(ctx, cs)
    T0, s0 = first_poses(n, 7) if given else (None, None)
    VO.window_poses(ctx, T0, s0)
    got = VO.window_poses_fetch(ctx)
    assert_chain_equal(got, WS.seq_chain(seq, T0, s0, R, t, scale))
    assert (got["status"] == VO.WP_OK).all()
    v = VO.window_poses_view(ctx)
    assert (v.n_windows, v.window_len) == (n, L) and v.poses6 and v.poses4x4 and v.status
    # a range of the block
    part = VO.window_poses_fetch(ctx, n - 1, 1)
    assert all(WS.bits_equal(part[k], got[k][n - 1:]) for k in got)
    # without T0 the first pose is the identity and its block zero
    if not given:
        assert (got["poses4x4"][:, 0] == np.eye(4)).all() and (got["poses6"][:, 0] == 0).all()


def test_the_cases_hold_what_the_chain_has_to_meet(ctx):
    """dead windows and pairs of four points come out as the degenerate pose (R = I, t = 0): the chain stands still"""
    seen_L, degenerate, moving, windows = set(), 0, 0, set()
    for name in CHAIN_CASES:
        cs = CASES[name]
        _, (R, t, _) = posed(ctx, cs)
        seen_L.add(cs["L"]), windows.add(len(cs["seen"]))
        still = (R.reshape(-1, 9) == I9).all(axis=1) & (t.reshape(-1, 3) == 0).all(axis=1)
        degenerate, moving = degenerate + int(still.sum()), moving + int((~still).sum())
    assert seen_L == {2, 3, 5} and min(windows) <= 2 and max(windows) == 7 and degenerate >= 5 and moving >= 10


def test_a_nan_in_the_tracks_is_the_degenerate_pose_not_a_nonfinite_window(pkg, ctx, seq):
    """the relative pose (rank 5) answers a pair whose points are not finite with the degenerate pose, so the chain of
    such a window is finite and stands still over that pair; ORBX_WP_NONFINITE is reached through overflow (below)
    and, for NaN motions, on the CPU (tests/test_window_poses_ref.py)"""
    VO, cs = pkg.orbx_vo, CASES["cap63"]
    tracks = cs["tracks"].copy()
    tracks[0, :, 1, 0] = np.nan  # frame 1 of window 0: pairs 0 and 1 of the window
    _, (R, t, scale) = posed(ctx, cs, tracks=tracks)
    assert (R[0, :2].reshape(-1, 9) == I9).all() and (t[0, :2] == 0).all() and np.isfinite(scale).all()
    VO.window_poses(ctx)
    got = VO.window_poses_fetch(ctx)
    assert got["status"].tolist() == [VO.WP_OK] * 3
    assert_chain_equal(got, WS.seq_chain(seq, None, None, R, t, scale))
    assert WS.bits_equal(got["poses4x4"][0, 2], got["poses4x4"][0, 0])


def test_an_overflowing_window_is_nonfinite_and_a_bad_pose_for_the_build(pkg, ctx, seq):
    """finite T0 and scale0 whose product is not: window 1 is ORBX_WP_NONFINITE, the others are untouched by it, and
    the chained build makes it ORBX_LM_BAD_POSE without a landmark -- the block of the host build with a pose beyond
    1e5 rad in its place"""
    VO, cs = pkg.orbx_vo, CASES["cap63"]
    n, L, cap = len(cs["seen"]), cs["L"], cs["cap"]
    (t_dev, s_dev), (R, t, scale) = posed(ctx, cs)
    assert np.abs(t[1, 0]).max() > 0.1  # pair 0 of window 1 moves
    T0, s0 = first_poses(n, 11)
    T0[1, :3, :3] *= 1e200
    s0[1] = 1e200
    VO.window_poses(ctx, T0, s0)
    got, ref = VO.window_poses_fetch(ctx), WS.seq_chain(seq, T0, s0, R, t, scale)
    assert got["status"].tolist() == ref["status"].tolist() == [VO.WP_OK, VO.WP_NONFINITE, VO.WP_OK]
    assert not np.isfinite(got["poses4x4"][1]).all()
    assert_chain_equal(got, ref, windows=[0, 2])
    VO.landmarks_build_chained(ctx, cs["K"], t_dev, s_dev)
    chained = ctx.landmarks_fetch()
    assert chained["status"][1] == pkg.orbx.LM_BAD_POSE and chained["point_offset"][1] == chained["point_offset"][2]
    poses = got["poses6"].copy()
    poses[1] = 0.0
    poses[1, :, 0] = 2e5
    ctx.landmarks_build(cs["K"], t_dev, s_dev, poses)
    LS.assert_blocks_equal(chained, ctx.landmarks_fetch())


# ---- 2. build -------------------------------------------------------------------------------------------------------
def test_chained_build_and_solve_equal_the_host_route(pkg, ctx):
    VO, cs = pkg.orbx_vo, CASES["cap257"]
    n = len(cs["seen"])
    (t_dev, s_dev), _ = posed(ctx, cs)
    T0, s0 = first_poses(n, 3)
    T0[1, :3, :3] = LR.rot_x(180.0)  # window 1 looks down the world's -z: no landmark passes z > 0
    VO.window_poses(ctx, T0, s0)
    poses6 = VO.window_poses_fetch(ctx)["poses6"]
    VO.landmarks_build_chained(ctx, cs["K"], t_dev, s_dev)
    chained = ctx.landmarks_fetch()
    ctx.bundle_adjust_landmarks(max_iters=50)
    solved = ctx.bundle_adjust_landmarks_fetch()
    status = chained["status"].tolist()
    assert status[1] == LR.EMPTY and status[3] == status[4] == LR.BASELINE and status.count(LR.OK) >= 3, status
    assert np.diff(chained["point_offset"])[np.array(status) == LR.OK].max() > 50
    # the route this replaces: the blocks fetched and handed back from the host
    ctx.landmarks_build(cs["K"], t_dev, s_dev, poses6)
    LS.assert_blocks_equal(chained, ctx.landmarks_fetch())
    ctx.bundle_adjust_landmarks(max_iters=50)
    host = ctx.bundle_adjust_landmarks_fetch()
    assert WS.bits_equal(solved[0], host[0]) and solved[1] == host[1] and WS.bits_equal(solved[2], host[2])
    assert sum(s["termination"] != pkg.orbx.BA_SKIPPED for s in solved[1]) == status.count(LR.OK)
    assert any(s["iterations"] >= 1 for s in solved[1])


def test_chained_build_refuses_other_sizes(pkg, ctx):
    VO, cs = pkg.orbx_vo, CASES["cap5"]
    (t_dev, s_dev), _ = posed(ctx, cs)
    VO.window_poses(ctx)
    VO.landmarks_build_chained(ctx, cs["K"], t_dev, s_dev)
    before = ctx.landmarks_fetch()
    for sizes in ((1, 5, 3), (2, 5, 2)):
        with pytest.raises(pkg.OrbxError) as e:
            VO.landmarks_build_chained(ctx, cs["K"], t_dev.data_ptr(), s_dev.data_ptr(), *sizes)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
    LS.assert_blocks_equal(ctx.landmarks_fetch(), before)


# ---- 3. gate --------------------------------------------------------------------------------------------------------
def ba_write_back_decides(mirror, tmp_path, solved, built):
    n, W = solved.shape[:2]
    path = tmp_path / "gate.bin"
    path.write_bytes(np.int32(n).tobytes() + np.int32(W).tobytes() + np.ascontiguousarray(solved).tobytes() +
                     np.ascontiguousarray(built).tobytes())
    r = subprocess.run([mirror, "gate", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.array([[int(v) for v in ln.split()[2:]] for ln in r.stdout.splitlines()], np.uint8)


@pytest.mark.parametrize("iters", WR.GATE_ITERS)
def test_gate_equals_the_sequential_restatement_and_ba_write_back(pkg, ctx, seq, mirror, tmp_path, iters):
    VO = pkg.orbx_vo
    built, tracks, seen = WR.gate_scenes()
    ctx.landmarks_build(LR.K_KITTI, tracks, seen, built)
    ctx.bundle_adjust_landmarks(max_iters=iters)
    solved, sums, _ = ctx.bundle_adjust_landmarks_fetch(points=False)
    term = np.array([s["termination"] for s in sums], np.int32)
    converged = iters > 1
    assert term.tolist() == [pkg.orbx.BA_CONVERGENCE if converged else pkg.orbx.BA_NO_CONVERGENCE] * 4 + \
        [pkg.orbx.BA_SKIPPED]
    free = np.zeros((5, WR.GATE_LEN), bool)
    free[:4, 1:] = True
    # the reference's thresholds
    VO.bundle_adjust_write_back(ctx)
    p4, upd = VO.bundle_adjust_write_back_fetch(ctx)
    r4, rupd, angle, dist = WS.seq_gate(seq, solved, built, term, WR.MAX_ROT_DIFF, WR.MAX_TRANS_DIFF)
    assert WS.bits_equal(p4, r4) and WS.bits_equal(upd, rupd)
    host = ba_write_back_decides(mirror, tmp_path, solved, built) * (term == pkg.orbx.BA_CONVERGENCE)[:, None]
    assert np.array_equal(upd, host.astype(np.uint8))
    v = VO.bundle_adjust_write_back_view(ctx)
    assert (v.n_windows, v.window_len) == (5, WR.GATE_LEN) and v.poses4x4 and v.updated
    if converged:
        assert upd[free].any() and not upd[free].all() and (angle[free] > WR.MAX_ROT_DIFF).any()
    else:
        assert not upd.any()  # whatever the one step moved, nothing is written back
    # a pose that is not updated is the inverse of the block as built, one that is, of the solved block
    old4 = WS.seq_gate(seq, built, built, np.full(5, pkg.orbx.BA_SKIPPED, np.int32), 1.0, 1.0)[0]
    assert WS.bits_equal(p4[upd == 0], old4[upd == 0])
    # thresholds between two poses' values: at least one pose on each side of each (generous ones without convergence)
    max_rot, max_trans = WR.mid_thresholds(angle, dist, free) if converged else (10.0, 1e6)
    for mr, mt in ((10.0, max_trans), (max_rot, 1e6)):
        VO.bundle_adjust_write_back(ctx, mr, mt)
        p4, upd = VO.bundle_adjust_write_back_fetch(ctx)
        r4, rupd, _, _ = WS.seq_gate(seq, solved, built, term, mr, mt)
        assert WS.bits_equal(p4, r4) and WS.bits_equal(upd, rupd)
        assert (upd[free].any() and not upd[free].all()) if converged else not upd.any()
    part = VO.bundle_adjust_write_back_fetch(ctx, 2, 2)
    assert WS.bits_equal(part[0], p4[2:4]) and WS.bits_equal(part[1], upd[2:4])


# ---- 4. state -------------------------------------------------------------------------------------------------------
@pytest.fixture()
def streams(pkg):
    hip = pkg.orbx.load()
    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    yield sa.value, sb.value
    assert hip.hipStreamDestroy(sa) == 0 and hip.hipStreamDestroy(sb) == 0


def flat(x):
    if isinstance(x, dict):
        return [(k, flat(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [flat(a) for a in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def test_refusals_leave_everything_as_it_was(pkg):
    VO, cs = pkg.orbx_vo, CASES["cap5"]
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        for call in (lambda: VO.window_poses(c), lambda: VO.window_poses_fetch(c),
                     lambda: VO.bundle_adjust_write_back(c), lambda: VO.bundle_adjust_write_back_fetch(c)):
            with pytest.raises(pkg.OrbxError) as e:  # nothing to chain, fetch or gate yet
                call()
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        (t_dev, s_dev), _ = posed(c, cs)
        T0, s0 = first_poses(2, 1)
        VO.window_poses(c, T0, s0)
        before = flat(VO.window_poses_fetch(c))
        bad_T0, bad_s0 = T0.copy(), s0.copy()
        bad_T0[1, 2, 3], bad_s0[0] = np.nan, np.inf
        for args in ((bad_T0, s0), (T0, bad_s0)):
            with pytest.raises(pkg.OrbxError) as e:
                VO.window_poses(c, *args)
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        with pytest.raises(pkg.OrbxError):
            VO.window_poses_fetch(c, 1, 2)
        assert flat(VO.window_poses_fetch(c)) == before
        # the gate: an unsolved block and bad thresholds
        VO.landmarks_build_chained(c, cs["K"], t_dev, s_dev)
        with pytest.raises(pkg.OrbxError) as e:
            VO.bundle_adjust_write_back(c)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        c.bundle_adjust_landmarks(max_iters=5)
        VO.bundle_adjust_write_back(c)
        kept = flat(VO.bundle_adjust_write_back_fetch(c))
        for bad in ((0.0, 50.0), (0.5, -1.0), (np.nan, 50.0), (0.5, np.inf)):
            with pytest.raises(pkg.OrbxError) as e:
                VO.bundle_adjust_write_back(c, *bad)
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        assert flat(VO.bundle_adjust_write_back_fetch(c)) == kept
        # a window longer than a solve takes
        long_tracks, long_seen = upload(np.zeros((1, 4, 9, 2), np.float32), np.zeros((1, 4), np.int32))
        c.tracks_pose(cs["K"], long_tracks, long_seen, max_iters=1)
        with pytest.raises(pkg.OrbxError) as e:
            VO.window_poses(c)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        assert flat(VO.window_poses_fetch(c)) == before


def whole_route(pkg, c, cs, T0, s0, streams):
    """tracks pose -> chain -> build -> solve -> gate, each stage on the next stream, no host wait in between"""
    VO = pkg.orbx_vo
    t_dev, s_dev = upload(cs["tracks"], cs["seen"])
    s = list(streams) + [None]
    c.tracks_pose(cs["K"], t_dev, s_dev, stream=s[0], **cs["kw"])
    VO.window_poses(c, T0, s0, stream=s[1])
    VO.landmarks_build_chained(c, cs["K"], t_dev, s_dev, stream=s[2])
    c.bundle_adjust_landmarks(max_iters=20, stream=s[0])
    VO.bundle_adjust_write_back(c, stream=s[1])
    out = (VO.bundle_adjust_write_back_fetch(c), VO.window_poses_fetch(c), c.landmarks_fetch(),
           c.bundle_adjust_landmarks_fetch(), c.tracks_pose_fetch())
    return flat(out), (t_dev, s_dev)


def test_caller_streams_growth_and_the_other_blocks(pkg, streams):
    """small, large, small on one context with every stage on another caller stream: each call equals the same call
    on a fresh context (the large one grows every block; the second small one runs in blocks larger than it needs),
    and the blocks of the other side paths are what they were"""
    order = [CASES["cap5"], CASES["cap257"], CASES["cap5"]]
    first = [first_poses(len(cs["seen"]), 20 + i) for i, cs in enumerate(order)]
    fresh = []
    for cs, (T0, s0) in zip(order, first):
        with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
            fresh.append(whole_route(pkg, c, cs, T0, s0, streams)[0])
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        for i, (cs, (T0, s0)) in enumerate(zip(order, first)):
            got, keep = whole_route(pkg, c, cs, T0, s0, streams[i % 2:] + streams[:i % 2])
            assert got == fresh[i], i
        # a chain and a gate change no other path's block
        others = lambda: flat((c.tracks_pose_fetch(), c.landmarks_fetch(), c.bundle_adjust_landmarks_fetch()))
        before = others()
        pkg.orbx_vo.window_poses(c, stream=streams[0])
        pkg.orbx_vo.bundle_adjust_write_back(c, 0.1, 1.0, stream=streams[1])
        pkg.orbx_vo.window_poses_fetch(c), pkg.orbx_vo.bundle_adjust_write_back_fetch(c)
        assert others() == before


def test_window_odometry_tracks_is_the_device_route_on_a_batch_of_one(pkg, ctx):
    VO = pkg.orbx_vo
    sc = LR.make_scene(700, W=5, slots=200, sigma=0.1, min_seen=2)
    T0, s0 = first_poses(1, 9)
    one = VO.window_odometry_tracks(ctx, LR.K_KITTI, sc["tracks"], sc["seen"], T0[0], s0[0])
    t_dev, s_dev = upload(sc["tracks"][None], sc["seen"][None])
    ctx.tracks_pose(LR.K_KITTI, t_dev, s_dev)
    VO.window_poses(ctx, T0, s0)
    VO.landmarks_build_chained(ctx, LR.K_KITTI, t_dev, s_dev)
    ctx.bundle_adjust_landmarks()
    VO.bundle_adjust_write_back(ctx)
    p4, upd = VO.bundle_adjust_write_back_fetch(ctx)
    assert WS.bits_equal(one["poses4x4"], p4[0]) and WS.bits_equal(one["updated"], upd[0])
    assert one["wp_status"] == VO.WP_OK and one["lm_status"] == ctx.landmarks_fetch()["status"][0] == LR.OK
    assert one["summary"] == ctx.bundle_adjust_landmarks_fetch(points=False)[1][0]
    assert one["summary"]["termination"] == pkg.orbx.BA_CONVERGENCE and upd[0].all()
