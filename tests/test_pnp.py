"""Perspective-n-point with RANSAC over the landmarks block on the device (include/orbx_pnp.h).
The device block -- records, seeded poses and masks -- is compared byte for byte with the sequential restatement
tests/cpp/pnp_sequential.cpp run on the FETCHED landmarks block (whose own parity tests/test_landmarks.py pins) and
the poses it was built with; the seeded solve bit for bit with orbx_bundle_adjust_batch on the fetched arrays.
Synthetic tracks are uploaded as arrays: no images.

The bound of test_what_the_seeds_buy, measured on the CPU with tests/cpp/ba_sequential.cpp from the same seeds (the
poses pnp_sequential gives, the landmarks lm_sequential gives): after the solve the poses of frames 2 .. 4 lie at most
SEEDED_ROT_MEASURED rad and SEEDED_T_MEASURED units from the true ones (float32 pixels) -> ten times that."""
import numpy as np
import pytest

import landmarks_ref as L
import landmarks_seq as LS
import pnp_ref as PR
import pnp_seq as S
import window_poses_ref as WR

pytestmark = pytest.mark.gpu
K = L.K_KITTI
CAP, W = 130, 5
PARAMS = dict(prob=0.99, threshold_px=0.5, max_iters=300, seed=17, refine_iters=10, min_inliers=4)
SEEDED_ROT_MEASURED, SEEDED_T_MEASURED = 1.4e-8, 2.5e-7  # measured: 1.38e-8 rad, 2.49e-7 units


def pad(sc, cap=CAP):
    """the scene with seen = 0 slots appended up to `cap`"""
    slots, w = sc["tracks"].shape[:2]
    out = dict(sc)
    out["tracks"] = np.concatenate([sc["tracks"], np.zeros((cap - slots, w, 2), np.float32)])
    out["seen"] = np.concatenate([sc["seen"], np.zeros(cap - slots, np.int32)])
    return out


def project(poses, X):
    """pixels (len(X), len(poses), 2) of world points under world -> camera angle-axis poses"""
    out = np.zeros((len(X), len(poses), 2))
    for k, p in enumerate(poses):
        q = X @ L.rodrigues(p[:3]).T + p[3:]
        out[:, k, 0] = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2]
        out[:, k, 1] = K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
    return out


def batch_scenes():
    """the one batch of test_bit_parity: (scenes, what each window is there for)"""
    rng = np.random.default_rng(71)
    scenes = [pad(L.make_scene(700 + w, W=W, slots=65, min_seen=W, pose_pert=0.002)) for w in range(3)]
    scenes.append(L.make_scene(703, W=W, slots=CAP, min_seen=W, outliers=0.3, pose_pert=0.002))
    baseline = pad(L.make_scene(704, W=W, slots=65, min_seen=W))
    baseline["poses"][1, 3:] = baseline["poses"][0, 3:] + np.array([0.01, 0.0, 0.02])
    scenes.append(baseline)
    three = pad(L.make_scene(705, W=W, slots=65, min_seen=W))
    three["seen"][3:] = 0
    three["tracks"][3:] = 0
    scenes.append(three)
    scenes.append(pad(L.make_scene(706, W=W, slots=100, min_seen=2)))  # seen of 2, 3, 4 and 5
    junk = pad(L.make_scene(707, W=W, slots=10, min_seen=W))
    junk["tracks"][:10, 3] = np.c_[rng.uniform(0, L.IMG_W, 10), rng.uniform(0, L.IMG_H, 10)]  # frame 3: all outliers
    scenes.append(junk)
    plane = pad(L.make_scene(708, W=W, slots=4, min_seen=W))
    pix = np.array([[300.0, 80.0, 1.0], [900.0, 100.0, 1.0], [350.0, 300.0, 1.0], [880.0, 290.0, 1.0]])
    plane["tracks"][:4] = project(plane["true_poses"], (np.linalg.inv(K) @ pix.T).T * 12.0)  # the plane z = 12
    scenes.append(plane)
    return scenes


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("pnp_seq_gpu"))


@pytest.fixture(scope="module")
def ba_seq(tmp_path_factory):
    return LS.compile_so(tmp_path_factory.mktemp("ba_seq_pnp"), "ba_sequential")


def build(ctx, scenes, **kw):
    poses, tracks, seen = L.stack(scenes)
    ctx.landmarks_build(K, tracks, seen, poses, **kw)
    return poses


def device(pkg, ctx, **params):
    pkg.orbx_pnp.window_poses_pnp(ctx, **params)
    return pkg.orbx_pnp.window_poses_pnp_fetch(ctx)


def assert_equal(got, ref, block):
    """records, seeded poses and masks, byte for byte"""
    assert got["records"].dtype == S.RECORD and got["records"].shape == ref["records"].shape
    for name in S.RECORD.names:
        assert got["records"][name].tobytes() == ref["records"][name].tobytes(), name
    assert got["records"].tobytes() == ref["records"].tobytes()
    assert got["poses6"].tobytes() == ref["poses6"].tobytes()
    n, per = ref["records"].shape
    for w in range(n):
        npts = block["point_offset"][w + 1] - block["point_offset"][w]
        for k in range(per):
            assert got["masks"][w][k].tobytes() == ref["mask"][w, k, :npts].tobytes(), (w, k)
            assert not ref["mask"][w, k, npts:].any()


def run_and_compare(pkg, ctx, seq, scenes, cap, **params):
    poses = build(ctx, scenes)
    block = ctx.landmarks_fetch()
    got = device(pkg, ctx, **params)
    ref = S.windows(seq, K, block, poses, cap, **params)
    assert_equal(got, ref, block)
    return got, ref, block, poses


def test_bit_parity_on_the_mixed_batch(pkg, ctx, seq):
    scenes = batch_scenes()
    got, ref, block, poses = run_and_compare(pkg, ctx, seq, scenes, CAP, **PARAMS)
    st, n = ref["records"]["status"], ref["records"]["n_corr"]
    # conditions on the reference: every case of the batch is what it is there for
    assert (st[:4] == S.OK).all() and (n[:3] == 65).all() and (n[3] == CAP).all()
    assert (ref["records"]["inliers"][:3] == 65).all()
    inl = ref["records"]["inliers"][3]
    assert (inl > 0.55 * CAP).all() and (inl < 0.85 * CAP).all()  # 30 % outliers
    assert (st[4] == S.SKIPPED).all() and block["status"][4] == L.BASELINE
    assert (st[5] == S.FEW_POINTS).all() and (n[5] == 3).all()
    assert (st[6] == S.OK).all() and n[6, 0] > n[6, 1] > n[6, 2] > 10  # seen of 3, 4, 5 thin out the later frames
    assert list(st[7]) == [S.OK, S.NO_MODEL, S.OK] and ref["records"]["iters"][7, 1] == PARAMS["max_iters"]
    assert ref["poses6"][7, 3].tobytes() == poses[7, 3].tobytes()  # the seeded pose equals the built one
    assert (st[8] == S.OK).all() and (n[8] == 4).all() and (ref["records"]["inliers"][8] == 4).all()
    for w in (4, 5):
        assert ref["poses6"][w].tobytes() == poses[w].tobytes()
    assert ref["poses6"][:, :2].tobytes() == poses[:, :2].tobytes()
    # the PnP poses are the true ones (poses 2 .. were handed out perturbed by 2e-3), up to the float32 pixels
    for w in (0, 1, 2, 3, 6):
        for k in range(2, W):
            er, et = PR.pose_error(got["poses6"][w, k], L.rodrigues(scenes[w]["true_poses"][k, :3]),
                                   scenes[w]["true_poses"][k, 3:])
            assert er < 1e-4 and et < 1e-2, (w, k, er, et)
    # the view
    v = pkg.orbx_pnp.window_poses_pnp_view(ctx)
    assert (v.n_windows, v.window_len, v.slot_capacity) == (len(scenes), W, CAP)
    # a range of the batch
    part = pkg.orbx_pnp.window_poses_pnp_fetch(ctx, 3, 4, masks=False)
    assert part["records"].tobytes() == ref["records"][3:7].tobytes()
    assert part["poses6"].tobytes() == ref["poses6"][3:7].tobytes()


@pytest.mark.parametrize("change", [dict(max_iters=0), dict(refine_iters=0), dict(refine_iters=20, min_inliers=30)])
def test_bit_parity_with_other_parameters(pkg, ctx, seq, change):
    scenes = batch_scenes()[2:5]
    params = dict(PARAMS, **change)
    got, ref, _, poses = run_and_compare(pkg, ctx, seq, scenes, CAP, **params)
    if params["max_iters"] == 0:
        assert (ref["records"]["status"][:2] == S.NO_MODEL).all() and (ref["records"]["iters"] == 0).all()
        assert ref["poses6"].tobytes() == poses.tobytes()
    else:
        assert (ref["records"]["status"][:2] == S.OK).all()


BIG = 513  # more than two workgroups' worth of lanes: every loop over the correspondences runs three times


@pytest.mark.parametrize("change", [dict(), dict(max_iters=64, prob=1.0)])
def test_bit_parity_beyond_one_workgroup_of_correspondences(pkg, ctx, seq, change):
    """257 and 513 live slots: the prologue's compaction carries its count across chunks, the scoring loop, the
    refinement's lane sums, the inlier counts and the mask clear all take a second and a third pass.  With
    max_iters = 64 under prob = 1 (no sample count ever suffices) the outlier window stops on the edge of the first
    chunk of 64 samples."""
    scenes = [pad(L.make_scene(740, W=W, slots=257, min_seen=W, pose_pert=0.002), BIG),
              L.make_scene(741, W=W, slots=BIG, min_seen=W, outliers=0.3, pose_pert=0.002)]
    params = dict(PARAMS, **change)
    got, ref, block, _ = run_and_compare(pkg, ctx, seq, scenes, BIG, **params)
    rec = ref["records"]
    assert (rec["status"] == S.OK).all()
    assert (rec["n_corr"][0] == 257).all() and (rec["inliers"][0] == 257).all()  # 256 < n_corr < cap
    assert (rec["n_corr"][1] == BIG).all()
    assert (rec["inliers"][1] > 256).all() and (rec["inliers"][1] < 0.85 * BIG).all()  # 30 % outliers
    assert any(ref["mask"][1, k, 256:].any() and not ref["mask"][1, k, 256:].all() for k in range(W - 2))
    if change:
        assert (rec["iters"][1] == 64).all() and (rec["iters"][0] < 64).all()
    else:
        assert (rec["iters"] < 64).all()
    for w in range(2):
        for k in range(2, W):
            er, et = PR.pose_error(got["poses6"][w, k], L.rodrigues(scenes[w]["true_poses"][k, :3]),
                                   scenes[w]["true_poses"][k, 3:])
            assert er < 1e-4 and et < 1e-2, (w, k, er, et)


def test_bit_parity_window_len_3(pkg, ctx, seq):
    """one problem per window"""
    scenes = [L.make_scene(720 + w, W=3, slots=65, min_seen=0, pose_pert=0.002) for w in range(4)]
    got, ref, _, _ = run_and_compare(pkg, ctx, seq, scenes, 65, **PARAMS)
    assert ref["records"].shape == (4, 1) and (ref["records"]["status"] == S.OK).all()
    assert (ref["records"]["n_corr"] < 40).all()  # seen in [0, 3]: about a quarter of the slots reach frame 2


def test_refusals(pkg, ctx):
    scenes2 = [L.make_scene(730, W=2, slots=20, min_seen=2)]
    build(ctx, scenes2)
    with pytest.raises(pkg.OrbxError):  # window_len 2: no later frame
        pkg.orbx_pnp.window_poses_pnp(ctx)
    build(ctx, [L.make_scene(731, W=3, slots=20, min_seen=3)])
    for bad in (dict(refine_iters=21), dict(refine_iters=-1), dict(min_inliers=3), dict(max_iters=-1),
                dict(max_iters=100001), dict(threshold_px=-1.0), dict(threshold_px=float("nan")),
                dict(prob=float("inf"))):
        with pytest.raises(pkg.OrbxError):
            pkg.orbx_pnp.window_poses_pnp(ctx, **dict(PARAMS, **bad))
    pkg.orbx_pnp.window_poses_pnp(ctx, **dict(PARAMS, prob=7.0))  # a finite prob is clamped
    with pytest.raises(pkg.OrbxError):
        pkg.orbx_pnp.window_poses_pnp_mask(ctx, 0, 3)  # k outside [2, window_len)
    build(ctx, [L.make_scene(732, W=3, slots=20, min_seen=3)])
    with pytest.raises(pkg.OrbxError):  # the seeds belong to the block before this one
        pkg.orbx_pnp.bundle_adjust_landmarks_pnp(ctx)


def test_batch_independence(pkg, ctx, seq):
    """70 windows of 8 slots -- many workgroups, tiny problems; window 37 gives the same bytes alone"""
    scenes = [L.make_scene(800 + w, W=W, slots=8, min_seen=3, pose_pert=0.002) for w in range(70)]
    got, ref, block, _ = run_and_compare(pkg, ctx, seq, scenes, 8, **PARAMS)
    st = ref["records"]["status"]
    assert list(st[37]) == [S.OK, S.OK, S.FEW_POINTS] and (st == S.OK).sum() > 140 and (st == S.FEW_POINTS).sum() > 40
    build(ctx, [scenes[37]])
    alone = device(pkg, ctx, **PARAMS)
    assert alone["records"][0].tobytes() == got["records"][37].tobytes()
    assert alone["poses6"][0].tobytes() == got["poses6"][37].tobytes()
    for k in range(W - 2):
        assert alone["masks"][0][k].tobytes() == got["masks"][37][k].tobytes()


def test_host_arrays_entry(pkg, ctx, seq):
    scenes = batch_scenes()[3:4]
    got, ref, block, _ = run_and_compare(pkg, ctx, seq, scenes, CAP, **PARAMS)
    pts, _, op, oq, xy = LS.window_of(block, 0)
    for k in (2, 4):
        sel = oq == k
        params = dict(PARAMS, seed=pkg.orbx_pnp.problem_seed(PARAMS["seed"], k))
        one = pkg.orbx_pnp.pnp_ransac(ctx, pts[op[sel]], xy[sel], K, **params)
        rec = got["records"][0, k - 2]
        assert one["pose6"].tobytes() == rec["pose6"].tobytes()
        assert (one["inliers"], one["iters"], one["status"]) == (rec["inliers"], rec["iters"], rec["status"])
        assert np.float64(one["rms_px"]).tobytes() == rec["rms_px"].tobytes()
        mask = np.zeros(len(pts), np.uint8)
        mask[op[sel]] = one["mask"]
        assert mask.tobytes() == got["masks"][0][k - 2].tobytes()
    # the batched block is still there behind the host entry
    again = pkg.orbx_pnp.window_poses_pnp_fetch(ctx)
    assert again["records"].tobytes() == got["records"].tobytes()
    # n = 0 and n = 3: FEW_POINTS
    assert pkg.orbx_pnp.pnp_ransac(ctx, np.zeros((0, 3)), np.zeros((0, 2)), K)["status"] == S.FEW_POINTS
    assert pkg.orbx_pnp.pnp_ransac(ctx, pts[:3], xy[:3], K)["status"] == S.FEW_POINTS


def test_a_refused_host_call_writes_nothing(pkg, ctx):
    import ctypes as C

    lib = pkg.orbx_pnp.load()
    X, uv, _, _ = PR.scene(5, n=20)
    X, uv, Kc = np.ascontiguousarray(X), np.ascontiguousarray(uv), np.ascontiguousarray(K)
    Kbad = Kc.copy()
    Kbad[0, 0] = 0.0
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    cases = [dict(K=Kbad), dict(K=None), dict(prob=float("nan")), dict(thr=-1.0), dict(thr=float("inf")),
             dict(max_iters=-1), dict(max_iters=100001), dict(n=-1), dict(refine=21), dict(refine=-1),
             dict(min_inliers=3), dict(pts=None), dict(pix=None)]
    for case in cases:
        pose, mask = np.full(6, 7.5), np.full(20, 9, np.uint8)
        inl, its, st, rms = C.c_int32(-5), C.c_int32(-5), C.c_int32(-5), C.c_double(-5.0)
        Kuse = case.get("K", Kc)
        rc = lib.orbx_pnp_ransac(ctx._h, dp(X) if "pts" not in case else None, dp(uv) if "pix" not in case else None,
                                 case.get("n", 20), None if Kuse is None else dp(Kuse), case.get("prob", 0.99),
                                 case.get("thr", 2.0), case.get("max_iters", 100), 0, case.get("refine", 10),
                                 case.get("min_inliers", 4), dp(pose), dp(mask), C.byref(inl), C.byref(its),
                                 C.byref(rms), C.byref(st))
        assert rc == pkg.orbx.ERR_INVALID_ARG, case
        assert (pose == 7.5).all() and (mask == 9).all(), case
        assert (inl.value, its.value, st.value, rms.value) == (-5, -5, -5, -5.0), case


def host_solve(ctx, block, poses, delta=1.0, max_iters=200):
    ok = [w for w in range(len(block["status"])) if block["status"][w] == L.OK]
    wins = []
    for w in ok:
        pts, _, op, oq, xy = LS.window_of(block, w)
        wins.append((poses[w], pts, op, oq, xy))
    return dict(zip(ok, ctx.bundle_adjust_batch(K, wins, huber_delta=delta, max_iters=max_iters)))


def test_seeded_solve_equals_the_host_entry_and_leaves_the_unseeded_one_alone(pkg, ctx):
    scenes = batch_scenes()
    poses = build(ctx, scenes)
    block = ctx.landmarks_fetch()
    ctx.bundle_adjust_landmarks()
    before = ctx.bundle_adjust_landmarks_fetch()
    got = device(pkg, ctx, **PARAMS)
    pkg.orbx_pnp.bundle_adjust_landmarks_pnp(ctx)
    sp, ss, sx = ctx.bundle_adjust_landmarks_fetch()
    ref = host_solve(ctx, block, got["poses6"])
    for w in range(len(scenes)):
        p0, p1 = block["point_offset"][w], block["point_offset"][w + 1]
        if w in ref:
            rp, rx, rs = ref[w]
            assert ss[w] == rs, (w, ss[w], rs)
            assert sp[w].tobytes() == rp.tobytes() and sx[p0:p1].tobytes() == rx.tobytes(), w
        else:
            assert ss[w]["termination"] == pkg.orbx.BA_SKIPPED and sp[w].tobytes() == got["poses6"][w].tobytes()
    # the seeds differ from the built poses, and so does the solve that starts from them
    assert ss[0]["initial_cost"] < before[1][0]["initial_cost"]
    # after a PnP call the unseeded solve still gives the bytes it gives without one, and the block stays as built
    ctx.bundle_adjust_landmarks()
    after = ctx.bundle_adjust_landmarks_fetch()
    assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1]
    assert after[2].tobytes() == before[2].tobytes()
    LS.assert_blocks_equal(ctx.landmarks_fetch(), block)


def chain_off_scale(true_poses, factor=1.5):
    """the window's world -> camera poses re-chained with the relative translations of pairs 1 .. multiplied by
    `factor` (pair 0, which the landmarks are built from, stays)"""
    T = []
    for p in true_poses:
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = L.rodrigues(p[:3]), p[3:]
        T.append(np.linalg.inv(M))  # camera -> world
    out = [T[0], T[1]]
    for k in range(2, len(T)):
        rel = np.linalg.inv(T[k - 1]) @ T[k]
        rel[:3, 3] *= factor
        out.append(out[-1] @ rel)
    poses = []
    for M in out:
        Mi = np.linalg.inv(M)
        poses.append(np.r_[L.rotvec(Mi[:3, :3]), Mi[:3, 3]])
    return np.array(poses)


def seeds_scene():
    sc = L.make_scene(900, W=W, slots=120, min_seen=W)
    sc["poses"] = chain_off_scale(sc["true_poses"])
    return sc


def worst_pose_error(poses, truth):
    e = [PR.pose_error(poses[k], L.rodrigues(truth[k, :3]), truth[k, 3:]) for k in range(2, len(truth))]
    return max(a for a, _ in e), max(b for _, b in e)


def test_what_the_seeds_buy(pkg, ctx, seq, ba_seq):
    sc = seeds_scene()
    poses = build(ctx, [sc])
    block = ctx.landmarks_fetch()
    assert block["status"][0] == L.OK
    ctx.bundle_adjust_landmarks()
    _, unseeded, _ = ctx.bundle_adjust_landmarks_fetch()
    got = device(pkg, ctx, **PARAMS)
    assert (got["records"]["status"] == S.OK).all()
    pkg.orbx_pnp.bundle_adjust_landmarks_pnp(ctx)
    sp, seeded, _ = ctx.bundle_adjust_landmarks_fetch()
    assert seeded[0]["initial_cost"] < unseeded[0]["initial_cost"]
    assert seeded[0]["initial_cost"] < 1e-3 < unseeded[0]["initial_cost"]  # float32 pixels against a chain off by 1.5
    # the CPU restatement from the same seeds
    pts, _, op, oq, xy = LS.window_of(block, 0)
    cp, _, cs = LS.seq_ba(ba_seq, K, got["poses6"][0], pts, op, oq, xy)
    cpu_rot, cpu_t = worst_pose_error(cp, sc["true_poses"])
    print("CPU restatement from the seeds: %.3e rad, %.3e units" % (cpu_rot, cpu_t))
    assert cpu_rot <= SEEDED_ROT_MEASURED and cpu_t <= SEEDED_T_MEASURED  # the measurement the bound stands on
    rot, t = worst_pose_error(sp[0], sc["true_poses"])
    print("device: %.3e rad, %.3e units" % (rot, t))
    assert rot <= 10 * SEEDED_ROT_MEASURED and t <= 10 * SEEDED_T_MEASURED
    # the write-back gate compares the solved poses against the poses the block was BUILT with, not against the seeds:
    # with max_trans = 0.05 the frames whose built pose is off by half a step stay as built
    pkg.orbx_vo.bundle_adjust_write_back(ctx, max_trans=0.05)
    _, updated = pkg.orbx_vo.bundle_adjust_write_back_fetch(ctx)
    _, want, _, dist = WR.gate(sp[0], poses[0], seeded[0]["termination"], max_trans=0.05)
    assert seeded[0]["termination"] == pkg.orbx.BA_CONVERGENCE and (dist[2:] > 0.2).all()
    assert list(updated[0]) == list(want) == [1, 1, 0, 0, 0]
    _, against_seeds, _, _ = WR.gate(sp[0], got["poses6"][0], seeded[0]["termination"], max_trans=0.05)
    assert list(against_seeds) == [1] * W


def test_callers_stream_behind_a_build_on_another_stream(pkg, ctx, seq):
    import torch

    scenes = batch_scenes()[:4]
    _, ref, block, _ = run_and_compare(pkg, ctx, seq, scenes, CAP, **PARAMS)
    build(ctx, [L.make_scene(950, W=W, slots=CAP, min_seen=2)])  # another block in between
    device(pkg, ctx, **PARAMS)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    build(ctx, scenes, stream=s1.cuda_stream)
    pkg.orbx_pnp.window_poses_pnp(ctx, stream=s2.cuda_stream, **PARAMS)  # no synchronisation in between
    pkg.orbx_pnp.bundle_adjust_landmarks_pnp(ctx, stream=s1.cuda_stream)
    got = pkg.orbx_pnp.window_poses_pnp_fetch(ctx)
    assert_equal(got, ref, block)
    sp, ss, _ = ctx.bundle_adjust_landmarks_fetch()
    want = host_solve(ctx, block, got["poses6"])
    for w, (rp, _, rs) in want.items():
        assert ss[w] == rs and sp[w].tobytes() == rp.tobytes(), w
    torch.cuda.synchronize()
