"""The search by projection on the device (include/orbx_search.h).  The projection is compared
with the sequential restatement tests/cpp/search_sequential.cpp bit for bit and with tests/search_ref.py's numpy
projection within search_seq.TOLERANCE_PX, with equal states; the gated re-association with search_ref.py byte for
byte.  Shapes: 70 x 300 (one workgroup of queries, cells of a few slots), 513 x 256 and 257 x 513 (two and three
workgroups of queries per window, train sets beyond one chunk of the sort's workgroup), a 96 x 64 frame and a
1241 x 40 strip (a grid of one row of cells and a long one), radii below one pixel, of 8 and beyond the frame."""
import numpy as np
import pytest

import carry_ref as CR
import landmarks_ref as L
import reassoc_ref as R
import search_ref as S
import search_seq as Q

pytestmark = pytest.mark.gpu
K = CR.K
W, H, MARGIN, CAP = S.IMG_W, S.IMG_H, S.PROJ_MARGIN, S.PROJ_CAP
PNP = dict(prob=0.99, threshold_px=0.5, max_iters=300, seed=17, refine_iters=10, min_inliers=4)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return Q.compile_so(tmp_path_factory.mktemp("search_seq_gpu"))


def bytes_equal(got, ref, keys=("xy", "depth", "state", "count")):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), k


def near_numpy(got, block, poses6, points=None):
    """equal states and counts, xy and depth within the measured tolerance; the scene keeps numpy clear of every state
    boundary, so no slot is left out"""
    detail = []
    ref = S.project(block, poses6, K, W, H, MARGIN, CAP, points=points, detail=detail)
    assert S.boundary_distance(detail, W, H, MARGIN) > 1e-6
    assert got["state"].tolist() == ref["state"].tolist() and got["count"].tolist() == ref["count"].tolist()
    assert np.abs(got["xy"] - ref["xy"]).max() <= Q.TOLERANCE_PX
    assert np.abs(got["depth"] - ref["depth"]).max() <= Q.TOLERANCE_PX
    return ref


def test_projection_parity(pkg, ctx, seq):
    o = pkg.orbx_search
    sc = S.projection_scene()
    poses, tracks, seen = CR.stack_old(sc["olds"])
    ctx.landmarks_build(K, tracks, seen, poses)
    block = ctx.landmarks_fetch()
    # the source as built, one pose per window, stride 6
    o.landmarks_project(ctx, K, sc["poses6"], W, H, MARGIN)
    got = o.landmarks_project_fetch(ctx)
    bytes_equal(got, Q.project(seq, block, sc["poses6"], K, W, H, MARGIN, CAP))
    S.check_projection_scene(block, near_numpy(got, block, sc["poses6"]))
    v = o.landmarks_project_view(ctx)
    assert (v.n_windows, v.slot_capacity) == (5, CAP) and v.xy and v.depth and v.state and v.count
    part = o.landmarks_project_fetch(ctx, 3, 2)
    assert all(part[k].tobytes() == got[k][3:].tobytes() for k in got)
    # one window on host arrays: the same bytes, as a projection of one window
    for w in (0, 4):
        p0, p1 = block["point_offset"][w], block["point_offset"][w + 1]
        one = o.project_landmarks_host(ctx, block["points3"][p0:p1], block["slot_of_point"][p0:p1], CAP, K,
                                       sc["poses6"][w], W, H, MARGIN)
        assert all(one[k].tobytes() == got[k][w].tobytes() for k in ("xy", "depth", "state")) and one["count"] == got["count"][w]
        assert o.landmarks_project_view(ctx).n_windows == 1
    none = o.project_landmarks_host(ctx, np.zeros((0, 3)), np.zeros(0, np.int32), 7, K, sc["poses6"][0], W, H, 0.0)
    assert none["count"] == 0 and not none["state"].any() and not none["xy"].any()
    # the solved source
    with pytest.raises(pkg.OrbxError):
        o.landmarks_project(ctx, K, sc["poses6"], W, H, MARGIN, source=CR.CARRY_SOLVED)  # not solved yet
    ctx.bundle_adjust_landmarks()
    _, _, solved = ctx.bundle_adjust_landmarks_fetch()
    assert solved.tobytes() != block["points3"].tobytes()
    o.landmarks_project(ctx, K, sc["poses6"], W, H, MARGIN, source=CR.CARRY_SOLVED)
    got_s = o.landmarks_project_fetch(ctx)
    bytes_equal(got_s, Q.project(seq, block, sc["poses6"], K, W, H, MARGIN, CAP, points=solved))
    near_numpy(got_s, block, sc["poses6"], points=solved)
    assert got_s["xy"].tobytes() != got["xy"].tobytes()
    # the last pose of every window of a carried PnP, read in place: stride 6 * window_len
    origin, ntracks, nseen = CR.stack_new(sc["news"])
    pkg.orbx_carry.landmarks_carry(ctx, origin)
    pkg.orbx_carry.window_poses_pnp_carried(ctx, K, ntracks, nseen, **PNP)
    pv = pkg.orbx_carry.window_poses_pnp_carried_view(ctx)
    assert (pv.n_windows, pv.window_len) == (5, S.PROJ_W)
    o.landmarks_project(ctx, K, pv.poses6 + 8 * 6 * (pv.window_len - 1), W, H, MARGIN, n_windows=5,
                        pose_stride=6 * pv.window_len)
    got_p = o.landmarks_project_fetch(ctx)
    carried = pkg.orbx_carry.window_poses_pnp_carried_fetch(ctx, masks=False)
    assert carried["window_status"].tolist() == [0, 0, 0, 1, 0]
    last = np.ascontiguousarray(carried["poses6"][:, -1])
    bytes_equal(got_p, Q.project(seq, block, last, K, W, H, MARGIN, CAP))
    bytes_equal(got_p, Q.project(seq, block, carried["poses6"].reshape(-1)[6 * (S.PROJ_W - 1):], K, W, H, MARGIN, CAP,
                                 pose_stride=6 * S.PROJ_W))
    ref = near_numpy(got_p, block, last)
    assert (ref["count"][[0, 1, 2, 4]] >= 10).all() and ref["count"][3] == 0


def upload_sets(g, lk_shaped=True):
    """the sets on the device; the query positions inside an array shaped like an LK view of five frames, in its
    frame 3 (point_stride 10)"""
    import torch

    n, qcap = g["qstate"].shape
    tracks = np.full((n, qcap, 5, 2), -7.0, np.float32)
    tracks[:, :, 3] = g["qxy"]
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("qdesc", "qstate", "tdesc", "tstate", "txy",
                                                                            "tpstate")}
    dev["qxy"] = torch.from_numpy(tracks).cuda()[:, :, 3] if lk_shaped else torch.from_numpy(g["qxy"]).cuda()
    torch.cuda.synchronize()
    return dev


def run_gated(pkg, ctx, dev, pstate=True, **params):
    o = pkg.orbx_search
    o.reassociate_gated(ctx, dev["qdesc"], dev["qstate"], dev["qxy"], dev["tdesc"], dev["tstate"], dev["txy"],
                        dev["tpstate"] if pstate else None, **params)
    got = pkg.orbx_reloc.reassociate_fetch(ctx)
    got["candidates"] = o.reassociate_gated_fetch(ctx)
    return got


def assert_gated(got, ref, what):
    for k in ("origin", "dist", "count", "candidates"):
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape, (what, k)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k)


COMBOS = [dict(unique=0, accept_lone=0, ratio=0.8, max_distance=40), dict(unique=1, accept_lone=1, ratio=0.8, max_distance=40),
          dict(unique=1, accept_lone=0, ratio=1.0, max_distance=256), dict(unique=0, accept_lone=1, ratio=1.0, max_distance=256)]


@pytest.mark.parametrize("frame", [(96, 64), (1241, 40)])
@pytest.mark.parametrize("qcap,tcap", [(70, 300), (513, 256), (257, 513)])
def test_gated_parity(pkg, ctx, qcap, tcap, frame):
    g = S.gated_windows(qcap, tcap, frame, 41 + qcap)
    dev = upload_sets(g)
    sets = (g["qdesc"], g["qstate"], g["qxy"], g["tdesc"], g["tstate"], g["txy"])
    seen_clump = seen_empty = seen_lone = False
    for radius in (0.75, 8.0, 3000.0):
        for p in COMBOS:
            params = dict(p, radius_px=radius)
            ref = S.reassociate_gated(*sets, g["tpstate"], **params)
            assert_gated(run_gated(pkg, ctx, dev, **params), ref, (radius, p))
            cand = ref["candidates"]
            seen_clump |= cand[1].max() > 256
            seen_empty |= bool((cand[0][g["qstate"][0] == R.PD_OK] == 0).any())
            seen_lone |= bool(((cand == 1) & (ref["origin"] >= 0)).any())
            assert ref["count"][2] == 0 and not cand[2].any()  # no positioned train slot
        if radius == 8.0:
            assert ref["count"][0] > 5 and ref["count"][3] > 5
    # the cases are what they are there for: a clump of more than 256 train slots inside one gate (where the train
    # set has that many), queries without a candidate, and lone candidates that accept_lone took
    assert seen_clump == (tcap >= 300) and seen_empty and seen_lone
    v = pkg.orbx_search.reassociate_gated_view(ctx)
    assert (v.n_windows, v.q_capacity) == (4, qcap) and v.candidates
    rv = pkg.orbx_reloc.reassociate_view(ctx)
    assert (rv.n_windows, rv.q_capacity, rv.t_capacity) == (4, qcap, tcap)
    # d_train_pstate NULL: every train slot with a finite position is positioned (window 2 has candidates now)
    params = dict(COMBOS[1], radius_px=8.0)
    ref = S.reassociate_gated(*sets, None, **params)
    got = run_gated(pkg, ctx, dev, pstate=False, **params)
    assert_gated(got, ref, "no pstate")
    assert ref["candidates"][2].any() and ref["count"][2] > 5
    part = pkg.orbx_search.reassociate_gated_fetch(ctx, 1, 2)
    assert part.tobytes() == ref["candidates"][1:3].tobytes()
    # one window on host arrays: the same rules, the blocks replaced by a batch of one
    for w, ps in ((0, g["tpstate"][0]), (1, None)):
        ref1 = S.reassociate_gated_window(*(a[w] for a in sets), ps, **params)
        one = pkg.orbx_search.reassociate_gated_host(ctx, *(a[w] for a in sets), ps, **params)
        assert one["origin"].tobytes() == ref1[0].tobytes() and one["dist"].tobytes() == ref1[1].tobytes()
        assert one["count"] == ref1[2] and one["candidates"].tobytes() == ref1[3].tobytes()
        assert pkg.orbx_search.reassociate_gated_view(ctx).n_windows == 1
    a = [x[0] for x in sets]
    none = pkg.orbx_search.reassociate_gated_host(ctx, a[0], a[1], a[2], a[3][:0], a[4][:0], a[5][:0], None, **params)
    assert (none["origin"] == -1).all() and not none["candidates"].any() and none["count"] == 0
    assert pkg.orbx_search.reassociate_gated_host(ctx, a[0][:0], a[1][:0], a[2][:0], a[3], a[4], a[5])["count"] == 0


def test_a_circle_over_the_whole_frame_is_the_ungated_call(pkg, ctx):
    qdesc, qstate, tdesc, tstate = R.synthetic_windows(70, 300)
    rng = np.random.default_rng(8)
    qxy = np.stack([rng.uniform(0, 1240, (3, 70)), rng.uniform(0, 375, (3, 70))], axis=-1).astype(np.float32)
    txy = np.stack([rng.uniform(0, 1240, (3, 300)), rng.uniform(0, 375, (3, 300))], axis=-1)
    for unique in (0, 1):
        for ratio, max_distance in ((0.8, 40), (1.0, 256)):
            pkg.orbx_reloc.reassociate(ctx, qdesc, qstate, tdesc, tstate, ratio=ratio, max_distance=max_distance,
                                       unique=unique)
            plain = pkg.orbx_reloc.reassociate_fetch(ctx)
            assert plain["count"][0] > 5
            pkg.orbx_search.reassociate_gated(ctx, qdesc, qstate, qxy, tdesc, tstate, txy, None, radius_px=5000.0,
                                              ratio=ratio, max_distance=max_distance, accept_lone=0, unique=unique)
            gated = pkg.orbx_reloc.reassociate_fetch(ctx)
            for k in ("origin", "dist", "count"):
                assert gated[k].tobytes() == plain[k].tobytes(), (unique, ratio, k)
            cand = pkg.orbx_search.reassociate_gated_fetch(ctx)
            want = (qstate == R.PD_OK) * (tstate == R.PD_OK).sum(axis=1)[:, None]
            assert cand.tolist() == want.tolist()


def test_repeated_structure(pkg, ctx):
    """every train descriptor twice, far apart: the ratio test alone accepts nothing, the gate accepts every query with
    the right slot"""
    r = S.repeated_structure()
    n = len(r["right"])
    sets = (r["qdesc"], r["qstate"], r["qxy"], r["tdesc"], r["tstate"], r["txy"])
    pkg.orbx_reloc.reassociate(ctx, r["qdesc"], r["qstate"], r["tdesc"], r["tstate"], ratio=0.8, max_distance=256,
                               unique=1)
    plain = pkg.orbx_reloc.reassociate_fetch(ctx)
    assert plain["count"].tolist() == [0] and (plain["origin"] == -1).all()
    for lone in (0, 1):
        params = dict(radius_px=10.0, ratio=0.8, max_distance=256, accept_lone=lone, unique=1)
        pkg.orbx_search.reassociate_gated(ctx, *sets, None, **params)
        got = pkg.orbx_reloc.reassociate_fetch(ctx)
        got["candidates"] = pkg.orbx_search.reassociate_gated_fetch(ctx)
        assert got["count"].tolist() == [n] and got["origin"][0].tolist() == r["right"].tolist()
        assert got["dist"][0].tolist() == [q % 7 for q in range(n)] and got["candidates"][0].tolist() == [2] * n
        assert_gated(got, S.reassociate_gated(*sets, None, **params), lone)


def descriptors_of(ids, seed):
    """one seeded descriptor per world point id, -1 (padding) random"""
    bank = np.random.default_rng(seed).integers(0, 256, (4096, 32), dtype=np.uint8)
    return bank[np.asarray(ids) % 4096]


def test_end_to_end_on_the_device(pkg, ctx):
    """generation 0 built; generation 1 carried by its tracked origin, localised and built; its landmarks projected
    under its own last PnP pose, read in place; generation 2 joined to it by the GATED re-association of synthetic
    descriptors, carried on that origin and localised -- no fetch before the end.  The carried count and the poses
    equal the route through the host entries, and the gated origin is the tracked one wherever a landmark exists."""
    import torch

    o, cy = pkg.orbx_search, pkg.orbx_carry
    Wn, slots, n = 4, 60, 2
    wins = CR.scale_streams(n_streams=n, W=Wn, slots=slots, gens=3, dying=10, seed=2150)
    stack = lambda g, k: np.stack([w[k] for w in wins[g]])
    ctx.landmarks_build(K, stack(0, "tracks"), stack(0, "seen"), stack(0, "true_poses"))
    cy.landmarks_carry(ctx, stack(1, "origin"))
    cy.window_poses_pnp_carried(ctx, K, stack(1, "tracks"), stack(1, "seen"), **PNP)
    cy.landmarks_build_carried(ctx, K, stack(1, "tracks"), stack(1, "seen"))
    pv = cy.window_poses_pnp_carried_view(ctx)
    o.landmarks_project(ctx, K, pv.poses6 + 8 * 6 * (Wn - 1), W, H, MARGIN, n_windows=n, pose_stride=6 * Wn)
    proj = o.landmarks_project_view(ctx)
    # banks: generation 1's slots (train) and generation 2's (query), a descriptor per world point, a few bits flipped
    rng = np.random.default_rng(12)
    tdesc = np.stack([descriptors_of(w["ids"], 3) for w in wins[1]])
    qdesc = np.stack([descriptors_of(w["ids"], 3) for w in wins[2]])
    for w in range(n):
        for q in range(slots):
            qdesc[w, q] = R.flip(qdesc[w, q], rng, int(rng.integers(0, 20)))
    state = np.full((n, slots), R.PD_OK, np.int32)
    tracks2 = torch.from_numpy(stack(2, "tracks")).cuda()
    seen2 = torch.from_numpy(stack(2, "seen")).cuda()
    torch.cuda.synchronize()
    params = dict(radius_px=6.0, ratio=0.8, max_distance=64, accept_lone=1, unique=1)
    o.reassociate_gated(ctx, qdesc, state, tracks2[:, :, 0], tdesc, state, proj.xy, proj.state, n_windows=n,
                        t_capacity=slots, **params)
    rv = pkg.orbx_reloc.reassociate_view(ctx)
    cy.landmarks_carry(ctx, rv.origin, n_windows=n, slot_capacity=rv.q_capacity)
    # (the projection read the carried PnP's block; the next carried PnP replaces it behind it on the same stream)
    cy.window_poses_pnp_carried(ctx, K, tracks2, seen2, **PNP)
    # ---- the end: everything is fetched now
    gen2 = cy.window_poses_pnp_carried_fetch(ctx, masks=False)
    carry = cy.landmarks_carry_fetch(ctx)
    origin = pkg.orbx_reloc.reassociate_fetch(ctx)["origin"]
    block = ctx.landmarks_fetch()
    projected = o.landmarks_project_fetch(ctx)
    assert (block["status"] == L.OK).all() and (gen2["window_status"] == 0).all() and (carry["count"] >= 30).all()
    # ---- the route through the host entries, from generation 0 on
    ctx.landmarks_build(K, stack(0, "tracks"), stack(0, "seen"), stack(0, "true_poses"))
    block0 = ctx.landmarks_fetch()
    for w in range(n):
        a0, a1 = block0["point_offset"][w], block0["point_offset"][w + 1]
        gen1 = cy.localise_carried_window(ctx, block0["points3"][a0:a1], block0["slot_of_point"][a0:a1],
                                          wins[1][w]["origin"], wins[1][w]["tracks"], wins[1][w]["seen"], K, **PNP)
        assert gen1["window_status"] == 0
        p0, p1 = block["point_offset"][w], block["point_offset"][w + 1]
        pts, slot = block["points3"][p0:p1], block["slot_of_point"][p0:p1]
        hp = o.project_landmarks_host(ctx, pts, slot, slots, K, gen1["poses6"][-1], W, H, MARGIN)
        assert all(hp[k].tobytes() == projected[k][w].tobytes() for k in ("xy", "depth", "state"))
        hg = o.reassociate_gated_host(ctx, qdesc[w], state[w], wins[2][w]["tracks"][:, 0], tdesc[w], state[w], hp["xy"],
                                      hp["state"], **params)
        assert hg["origin"].tobytes() == origin[w].tobytes()
        hl = cy.localise_carried_window(ctx, pts, slot, hg["origin"], wins[2][w]["tracks"], wins[2][w]["seen"], K, **PNP)
        assert (hl["carried_point"] >= 0).sum() == carry["count"][w]
        assert hl["carried_point"].tobytes() == carry["point"][w].tobytes()
        assert hl["poses6"].tobytes() == gen2["poses6"][w].tobytes() and hl["window_status"] == 0
        # the gate found the tracked origin wherever the old slot's landmark was projected into the frame
        tracked = wins[2][w]["origin"]
        there = (tracked >= 0) & (projected["state"][w][np.maximum(tracked, 0)] == S.PROJ_OK)
        assert there.sum() >= 30 and (origin[w][there] == tracked[there]).all()


def test_callers_streams(pkg, ctx, seq):
    """the projection on one stream, the descriptors on a second and the gated re-association on a third, with no
    synchronisation in between: every call waits on the device for the block it reads; the bytes are those of the run
    on the context's own stream"""
    import torch

    o, rl = pkg.orbx_search, pkg.orbx_reloc
    sc = S.projection_scene()
    poses, tracks, seen = CR.stack_old(sc["olds"])
    ctx.landmarks_build(K, tracks, seen, poses)
    rng = np.random.default_rng(21)
    frames = torch.from_numpy(rng.integers(0, 256, (5, 160, 320), dtype=np.uint8)).cuda()
    pts = [torch.from_numpy(np.stack([rng.uniform(20, 299, (5, CAP)), rng.uniform(20, 139, (5, CAP))],
                                     axis=-1).astype(np.float32)).cuda() for _ in range(2)]
    poses6 = torch.from_numpy(sc["poses6"]).cuda()
    torch.cuda.synchronize()
    params = dict(radius_px=400.0, ratio=1.0, max_distance=256, accept_lone=1, unique=1)

    def run(streams):
        s = [x.cuda_stream if x is not None else None for x in streams]
        o.landmarks_project(ctx, K, poses6, W, H, MARGIN, stream=s[0])
        for bank in (0, 1):
            rl.describe_points(ctx, frames, pts[bank], bank=bank, stream=s[1])
        pv = o.landmarks_project_view(ctx)
        o.reassociate_gated(ctx, rl.point_descriptors_view(ctx, 1), None, pts[1], rl.point_descriptors_view(ctx, 0), None,
                            pv.xy, pv.state, stream=s[2], **params)
        got = rl.reassociate_fetch(ctx)
        got["candidates"] = o.reassociate_gated_fetch(ctx)
        return got

    own = run([None, None, None])
    assert own["count"][4] >= 3 and own["candidates"][4].max() >= 2 and own["count"][1:4].tolist() == [0, 0, 0]
    three = run([torch.cuda.Stream() for _ in range(3)])
    assert_gated(three, own, "streams")
    torch.cuda.synchronize()
    # and both are the reference on the fetched banks and projection
    q, t, proj = rl.point_descriptors_fetch(ctx, 1), rl.point_descriptors_fetch(ctx, 0), o.landmarks_project_fetch(ctx)
    ref = S.reassociate_gated(q["desc"], q["state"], pts[1].cpu().numpy(), t["desc"], t["state"], proj["xy"],
                              proj["state"], **params)
    assert_gated(own, ref, "reference")


def snapshot(pkg, ctx):
    out = dict(pkg.orbx_search.landmarks_project_fetch(ctx))
    out.update(("ra_" + k, v) for k, v in pkg.orbx_reloc.reassociate_fetch(ctx).items())
    out["candidates"] = pkg.orbx_search.reassociate_gated_fetch(ctx)
    return out


def test_argument_errors_write_nothing(pkg, ctx):
    import torch

    o = pkg.orbx_search
    sc = S.projection_scene()
    poses, tracks, seen = CR.stack_old(sc["olds"])
    ctx.landmarks_build(K, tracks, seen, poses)
    poses6 = torch.from_numpy(sc["poses6"]).cuda()
    g = S.gated_windows(70, 300, (96, 64), 41)
    dev = upload_sets(g, lk_shaped=False)
    good = dict(radius_px=8.0, ratio=0.8, max_distance=64, accept_lone=1, unique=1)
    o.landmarks_project(ctx, K, poses6, W, H, MARGIN)
    run_gated(pkg, ctx, dev, **good)
    before = snapshot(pkg, ctx)
    assert before["count"].sum() > 20 and before["ra_count"].sum() > 10 and before["candidates"].any()
    lib, h, bad = o.load(), ctx._h, pkg.orbx.ERR_INVALID_ARG
    Kc, P = np.ascontiguousarray(K, np.float64), poses6.data_ptr()

    def project(K_=Kc.ctypes.data, pose=P, stride=6, n=5, source=0, w=W, hh=H, margin=MARGIN):
        return lib.orbx_landmarks_project_device(h, K_, pose, stride, n, source, w, hh, margin, None)

    nan, inf = float("nan"), float("inf")
    Kbad = Kc.copy()
    Kbad[0, 0] = 0.0
    for kw in (dict(K_=None), dict(K_=Kbad.ctypes.data), dict(pose=None), dict(pose=P + 4), dict(stride=5), dict(n=4),
               dict(n=6), dict(source=2), dict(source=1), dict(w=0), dict(hh=0), dict(margin=-1.0), dict(margin=nan),
               dict(margin=inf)):
        assert project(**kw) == bad, kw
    a = dict(qd=dev["qdesc"].data_ptr(), qs=dev["qstate"].data_ptr(), qx=dev["qxy"].data_ptr(), ps=2, fs=140, qcap=70,
             td=dev["tdesc"].data_ptr(), ts=dev["tstate"].data_ptr(), tx=dev["txy"].data_ptr(),
             tp=dev["tpstate"].data_ptr(), tcap=300, n=4, radius=8.0, ratio=0.8, maxd=64, lone=1, unique=1)

    def gated(**kw):
        b = dict(a, **kw)
        return lib.orbx_reassociate_gated_device(h, b["qd"], b["qs"], b["qx"], b["ps"], b["fs"], b["qcap"], b["td"],
                                                 b["ts"], b["tx"], b["tp"], b["tcap"], b["n"], b["radius"], b["ratio"],
                                                 b["maxd"], b["lone"], b["unique"], None)

    for kw in (dict(qd=None), dict(qs=None), dict(td=None), dict(ts=None), dict(qd=a["qd"] + 8), dict(ts=a["ts"] + 2),
               dict(qx=None), dict(qx=a["qx"] + 2), dict(ps=1), dict(fs=139), dict(tx=None), dict(tx=a["tx"] + 4),
               dict(tp=a["tp"] + 2), dict(qcap=0), dict(tcap=0), dict(n=0), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=nan), dict(radius=inf), dict(ratio=-0.1), dict(ratio=nan), dict(maxd=-1), dict(maxd=257),
               dict(lone=2), dict(lone=-1), dict(unique=2)):
        assert gated(**kw) == bad, kw
    assert gated(n=65536) == pkg.orbx.ERR_UNSUPPORTED and gated(qcap=(1 << 22) + 1) == pkg.orbx.ERR_UNSUPPORTED
    # the host entries refuse the same parameters
    one = [g[k][0] for k in ("qdesc", "qstate", "qxy", "tdesc", "tstate", "txy")]
    for kw in (dict(radius_px=0.0), dict(accept_lone=2), dict(ratio=nan), dict(max_distance=300)):
        with pytest.raises(pkg.OrbxError):
            o.reassociate_gated_host(ctx, *one, None, **dict(good, **kw))
    with pytest.raises(pkg.OrbxError):
        o.project_landmarks_host(ctx, np.zeros((1, 3)), [0], 0, K, np.zeros(6), W, H, 0.0)
    with pytest.raises(pkg.OrbxError):
        o.project_landmarks_host(ctx, np.zeros((1, 3)), [0], 4, K, np.zeros(6), W, H, -2.0)
    # a fetch outside the blocks
    for call in (lambda: o.landmarks_project_fetch(ctx, 4, 2), lambda: o.reassociate_gated_fetch(ctx, 3, 2),
                 lambda: o.landmarks_project_fetch(ctx, -1, 1)):
        with pytest.raises(pkg.OrbxError):
            call()
    after = snapshot(pkg, ctx)
    assert sorted(after) == sorted(before)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    # the context is usable: the same calls give the same bytes
    o.landmarks_project(ctx, K, poses6, W, H, MARGIN)
    run_gated(pkg, ctx, dev, **good)
    again = snapshot(pkg, ctx)
    assert all(again[k].tobytes() == before[k].tobytes() for k in before)


def test_before_the_first_call_the_views_refuse(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160)) as c:
        for call in (pkg.orbx_search.landmarks_project_view, pkg.orbx_search.reassociate_gated_view,
                     pkg.orbx_search.landmarks_project_fetch, pkg.orbx_search.reassociate_gated_fetch):
            with pytest.raises(pkg.OrbxError):
                call(c)
        with pytest.raises(pkg.OrbxError):  # no landmarks block
            pkg.orbx_search.landmarks_project(c, K, np.zeros((1, 6)), W, H)
