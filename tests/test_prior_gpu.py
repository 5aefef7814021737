"""Landmark priors in the window solve on the device (include/orbx_prior.h).  k_ba_lm<true>
through orbx_bundle_adjust_prior_batch is compared bit for bit with the sequential restatement
(tests/cpp/ba_prior_sequential.cpp, which tests/test_ba_prior.py pins on the CPU); with every weight 0 with
Context.bundle_adjust_batch; the device route of a carried generation (rule P6's gather, then the solve of the
landmarks block) with the host route on the fetched arrays.  Synthetic windows and tracks: no images."""
import numpy as np
import pytest

import carry_ref as R
import landmarks_ref as L
import landmarks_seq as LS
import test_ba as B
from test_ba_prior import START_ANCHOR, START_GIVEN, mixed_priors, pseq, seq_ba_prior  # noqa: F401  (pseq: a fixture)

pytestmark = pytest.mark.gpu
K = R.K
PARAMS = R.MIX_PARAMS
SKIPPED = 3
WEIGHT = 1.0


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def mixed():
    return R.mixed_batch()


def tup(w):
    return (w["poses0"], w["pts0"], w["obs_point"], w["obs_pose"], w["obs_xy"])


def same(a, b):
    """poses, points and every summary field, bit for bit"""
    return B.same(a, b) and set(a[2]) == set(b[2])


# ---- 8. bit parity with the restatement --------------------------------------------------------------------------------
def parity_cases():
    """(name, window, anchors, weights): landmarks at the lane-stride boundaries of a 256-lane workgroup x every window
    length, pixel noise 0 and 0.3 in turn, one window with outliers, one whose first landmarks are seen once and carry
    a prior.  Weights are mixed per landmark from {0, 1e-2, 1, 1e6}; anchors are the truth + N(0, 0.1)."""
    cases, seed = [], 1100
    for n in (1, 7, 63, 256, 257, 513):
        for W in (2, 3, 5, 8):
            sigma = 0.3 if (seed % 2) else 0.0
            win = B.make_window(seed, W, n, sigma=sigma)
            cases.append(("n%d W%d s%g" % (n, W, sigma), win, *mixed_priors(win, seed + 500)))
            seed += 1
    win = B.make_window(seed, 5, 300, sigma=0.3, outliers=0.1)
    cases.append(("outliers", win, *mixed_priors(win, seed + 500)))
    win = B.make_window(seed + 1, 5, 120, sigma=0.3)
    keep = np.ones(len(win["obs_point"]), bool)
    for j in range(10):  # landmarks 0 .. 9 keep one observation only; the prior is what holds their depth
        keep[np.flatnonzero(win["obs_point"] == j)[1:]] = False
    win = {**win, "obs_point": win["obs_point"][keep], "obs_pose": win["obs_pose"][keep], "obs_xy": win["obs_xy"][keep]}
    anchors, weights = mixed_priors(win, seed + 501)
    weights[:10] = 1.0
    cases.append(("seen once with a prior", win, anchors, weights))
    return cases


@pytest.fixture(scope="module")
def cases():
    return parity_cases()


@pytest.mark.parametrize("start", [START_GIVEN, START_ANCHOR])
@pytest.mark.parametrize("delta", [1.0, 2.5])
def test_batch_equals_the_restatement_bit_for_bit(pkg, ctx, pseq, cases, start, delta):
    assert len(cases) == 26
    got = pkg.orbx_prior.bundle_adjust_prior_batch(ctx, B.K_KITTI, [tup(w) for _, w, _, _ in cases],
                                                   [(a, lam) for _, _, a, lam in cases], start, huber_delta=delta)
    terms = set()
    for (name, w, a, lam), g in zip(cases, got):
        assert set(lam) <= {0.0, 1e-2, 1.0, 1e6} and (len(lam) < 7 or len(set(lam)) > 1), name
        ref = seq_ba_prior(pseq, w, a, lam, start, delta=delta)
        terms.add(ref[2]["termination"])
        assert same(g, ref), (name, g[2], ref[2])
        if ref[2]["termination"] == B.CONVERGENCE and start == START_GIVEN:
            assert not np.array_equal(g[1], w["pts0"]), name
    assert B.CONVERGENCE in terms


def test_no_convergence_returns_the_given_blocks(pkg, ctx, pseq, cases):
    """max_iters = 1 under ORBX_PRIOR_START_ANCHOR: the solve ran from the anchors, and what comes back on
    `no_convergence` is the given blocks, not the anchors (rule P5)"""
    got = pkg.orbx_prior.bundle_adjust_prior_batch(ctx, B.K_KITTI, [tup(w) for _, w, _, _ in cases],
                                                   [(a, lam) for _, _, a, lam in cases], START_ANCHOR, max_iters=1)
    stopped = 0
    for (name, w, a, lam), g in zip(cases, got):
        ref = seq_ba_prior(pseq, w, a, lam, START_ANCHOR, max_iters=1)
        assert same(g, ref), (name, g[2], ref[2])
        if g[2]["termination"] == B.NO_CONVERGENCE:
            stopped += 1
            assert g[2]["iterations"] == 1
            assert g[0].tobytes() == np.ascontiguousarray(w["poses0"]).tobytes(), name
            assert g[1].tobytes() == np.ascontiguousarray(w["pts0"]).tobytes(), name
            # the cost it reports is the anchored start's, not the given one's
            given = seq_ba_prior(pseq, w, a, lam, START_GIVEN, max_iters=1)[2]
            assert given["initial_cost"] != g[2]["initial_cost"] or not (lam > 0).any(), name
    assert stopped >= len(cases) // 2


def test_single_window_entry_equals_the_batch(pkg, ctx, cases):
    name, w, a, lam = cases[17]  # 257 landmarks
    one = pkg.orbx_prior.bundle_adjust_prior(ctx, B.K_KITTI, *tup(w), a, lam, START_ANCHOR, huber_delta=2.5)
    many = pkg.orbx_prior.bundle_adjust_prior_batch(ctx, B.K_KITTI, [tup(w)], [(a, lam)], START_ANCHOR, huber_delta=2.5)
    assert len(w["pts0"]) == 257 and same(one, many[0])


# ---- 9. zero weights ---------------------------------------------------------------------------------------------------
def test_zero_weights_and_null_priors_equal_the_plain_solve(pkg, ctx, cases):
    """k_ba_lm<true> with every weight 0, and with no prior arrays at all, returns every byte of k_ba_lm<false>
    (Context.bundle_adjust_batch) on the same arrays, from both start modes"""
    pick = [c for c in cases if len(c[1]["pts0"]) in (7, 257, 513)] + cases[-2:]
    assert sum(len(c[1]["pts0"]) == 257 for c in pick) == 4
    wins = [tup(w) for _, w, _, _ in pick]
    plain = ctx.bundle_adjust_batch(B.K_KITTI, wins, max_iters=50)
    rng = np.random.default_rng(3)
    zero = [(rng.normal(0.0, 50.0, w["pts0"].shape), np.zeros(len(w["pts0"]))) for _, w, _, _ in pick]
    for start in (START_GIVEN, START_ANCHOR):
        for priors in (zero, None):
            got = pkg.orbx_prior.bundle_adjust_prior_batch(ctx, B.K_KITTI, wins, priors, start, max_iters=50)
            for (name, _, _, _), g, p in zip(pick, got, plain):
                assert same(g, p), (name, start, priors is None)
    assert {p[2]["termination"] for p in plain} >= {B.CONVERGENCE}


# ---- 10. batch independence --------------------------------------------------------------------------------------------
def test_batch_independence(pkg, ctx):
    """70 small windows in one call (more windows than a wave has lanes, every workgroup's workspace reused by none):
    window 37 alone gives the same bytes, and so does the batch with every OTHER window's anchors replaced"""
    wins = [B.make_window(1300 + k, 5, 8, sigma=0.3) for k in range(70)]
    priors = [mixed_priors(w, 1400 + k) for k, w in enumerate(wins)]
    op = pkg.orbx_prior
    got = op.bundle_adjust_prior_batch(ctx, B.K_KITTI, [tup(w) for w in wins], priors, START_ANCHOR)
    alone = op.bundle_adjust_prior_batch(ctx, B.K_KITTI, [tup(wins[37])], [priors[37]], START_ANCHOR)
    assert same(alone[0], got[37]) and (priors[37][1] > 0).any()
    rng = np.random.default_rng(9)
    other = [(a if k == 37 else rng.normal(0.0, 1e3, a.shape), lam) for k, (a, lam) in enumerate(priors)]
    again = op.bundle_adjust_prior_batch(ctx, B.K_KITTI, [tup(w) for w in wins], other, START_ANCHOR)
    assert same(again[37], got[37])
    assert sum(not same(x, y) for x, y in zip(again, got)) > 30  # (the garbage did reach the other windows)


# ---- 11. the device route equals the host route --------------------------------------------------------------------------
def numpy_priors(block, carry, weight):
    """rule P6 on the fetched landmarks block and the fetched carry block"""
    n = len(block["status"])
    total = int(block["point_offset"][n])
    xyz, lam, count = np.zeros((total, 3)), np.zeros(total), np.zeros(n, np.int32)
    for w in range(n):
        if block["status"][w] != L.OK:
            continue
        for p in range(int(block["point_offset"][w]), int(block["point_offset"][w + 1])):
            s = int(block["slot_of_point"][p])
            if carry["point"][w, s] >= 0:
                xyz[p], lam[p] = carry["xyz"][w, s], weight
                count[w] += 1
    return xyz, lam, count


def device_generation(pkg, ctx, olds, news, start, weight=WEIGHT, gather_stream=None, solve_stream=None):
    """carry -> carried PnP -> carried build -> priors -> solve, no fetch in between; then everything fetched"""
    oc, op = pkg.orbx_carry, pkg.orbx_prior
    poses, tracks, seen = R.stack_old(olds)
    ctx.landmarks_build(K, tracks, seen, poses)
    origin, tracks, seen = R.stack_new(news)
    oc.landmarks_carry(ctx, origin)
    oc.window_poses_pnp_carried(ctx, K, tracks, seen, **PARAMS)
    oc.landmarks_build_carried(ctx, K, tracks, seen)
    op.landmarks_priors_carried(ctx, weight, stream=gather_stream)
    op.bundle_adjust_landmarks_prior(ctx, start=start, stream=solve_stream)
    return dict(carry=oc.landmarks_carry_fetch(ctx), pnp=oc.window_poses_pnp_carried_fetch(ctx, masks=False),
                block=ctx.landmarks_fetch(), priors=op.landmarks_priors_fetch(ctx),
                solve=ctx.bundle_adjust_landmarks_fetch())


def check_against_host_route(pkg, ctx, dev, news, start, weight=WEIGHT):
    block, carry, pri = dev["block"], dev["carry"], dev["priors"]
    xyz, lam, count = numpy_priors(block, carry, weight)
    assert pri["prior_xyz"].tobytes() == xyz.tobytes() and pri["prior_weight"].tobytes() == lam.tobytes()
    assert pri["count"].dtype == np.int32 and pri["count"].tobytes() == count.tobytes()
    sp, ss, sx = dev["solve"]
    ok = [w for w in range(len(news)) if block["status"][w] == L.OK]
    for w in range(len(news)):
        p0, p1 = int(block["point_offset"][w]), int(block["point_offset"][w + 1])
        fresh = news[w]["origin"][block["slot_of_point"][p0:p1]] < 0
        assert not lam[p0:p1][fresh].any() and not xyz[p0:p1][fresh].any(), w  # fresh slots: weight 0, anchor 0
        if dev["pnp"]["window_status"][w] == R.CARRY_LOST:
            assert block["status"][w] != L.OK and count[w] == 0 and ss[w]["termination"] == SKIPPED, w
    wins = [(dev["pnp"]["poses6"][w], *[LS.window_of(block, w)[k] for k in (0, 2, 3, 4)]) for w in ok]
    pri_w = [(xyz[block["point_offset"][w]:block["point_offset"][w + 1]],
              lam[block["point_offset"][w]:block["point_offset"][w + 1]]) for w in ok]
    host = pkg.orbx_prior.bundle_adjust_prior_batch(ctx, K, wins, pri_w, start) if ok else []
    for w, (hp, hx, hs) in zip(ok, host):
        p0, p1 = int(block["point_offset"][w]), int(block["point_offset"][w + 1])
        assert ss[w] == hs, (w, ss[w], hs)
        assert sp[w].tobytes() == hp.tobytes() and sx[p0:p1].tobytes() == hx.tobytes(), w
    return count, ss


@pytest.mark.parametrize("start", [START_GIVEN, START_ANCHOR])
def test_device_route_equals_host_route_on_the_mixed_batch(pkg, ctx, mixed, start):
    """first the windows of tests/test_carry.py::test_build_and_solve_behind_it (all localised), then the whole mixed
    batch with its LOST windows"""
    pick = [0, 1, 2, 6, 7]
    olds, news = [[m[w] for w in pick] for m in mixed]
    dev = device_generation(pkg, ctx, olds, news, start)
    assert (dev["pnp"]["window_status"] == R.CARRY_OK).all() and (dev["block"]["status"] == L.OK).all()
    count, ss = check_against_host_route(pkg, ctx, dev, news, start)
    assert count[0] > 50 and (count > 0).all()
    assert any(s["termination"] == B.CONVERGENCE for s in ss) and all(s["termination"] != SKIPPED for s in ss)
    olds, news = mixed
    dev = device_generation(pkg, ctx, olds, news, start)
    lost = dev["pnp"]["window_status"] == R.CARRY_LOST
    assert list(np.flatnonzero(lost)) == [3, 4]
    count, ss = check_against_host_route(pkg, ctx, dev, news, start)
    assert not count[lost].any() and count[~lost].all()


@pytest.mark.parametrize("cap", [1, 63, 64, 65, 257])
def test_device_route_equals_host_route_at_slot_capacities(pkg, ctx, cap, start=START_ANCHOR):
    """two windows of `cap` slots each: the gather's workgroup boundary (256), the count's wave boundary (64) and a
    window of one slot, which cannot be localised and is skipped"""
    fresh = min(10, cap // 6)
    olds, news = [], []
    for k in range(2):
        _, old, new = R.two_generations(1600 + 10 * cap + k, R.MIX_W, cap - fresh, fresh, min_seen=R.MIX_W, cap=cap)
        olds.append(R._pad_old(old, cap)), news.append(new)
    dev = device_generation(pkg, ctx, olds, news, start)
    assert pkg.orbx_carry.landmarks_carry_view(ctx).slot_capacity == cap == ctx.landmarks_view().slot_capacity
    count, ss = check_against_host_route(pkg, ctx, dev, news, start)
    if cap == 1:
        assert not count.any() and all(s["termination"] == SKIPPED for s in ss)
    else:
        assert (count > (cap - fresh) // 2).all() and (count <= cap - fresh).all()
        assert all(s["termination"] in (B.CONVERGENCE, B.NO_CONVERGENCE) for s in ss)


# ---- 12. what it buys ----------------------------------------------------------------------------------------------------
# measured on the MI355X by this test (it prints them); the bounds are 10 x these
ANCHOR_MOVE_MEASURED = 1.94e-6   # largest |X - A| / |A| over the anchored landmarks of generations 1 and 2; measured: 1.939e-6
PRIOR_RATIO_MEASURED = 7.68e-7   # carry_ref.scale_deviation's length ratio, prior solve behind every build; measured: 7.673e-7


def scale_run(pkg, ctx, wins, with_priors):
    """test_carry.py::test_the_scale_stays with a solve behind every carried build, the solved points carried on"""
    oc, op = pkg.orbx_carry, pkg.orbx_prior
    stack = lambda g, key: np.stack([w[key] for w in wins[g]])
    ctx.landmarks_build(K, stack(0, "tracks"), stack(0, "seen"), np.stack([R.scaled(w["true_poses"], 3.0) for w in wins[0]]))
    results, move = [], 0.0
    for g in (1, 2):
        oc.landmarks_carry(ctx, stack(g, "origin"), source=R.CARRY_BUILT if g == 1 else R.CARRY_SOLVED)
        oc.window_poses_pnp_carried(ctx, K, stack(g, "tracks"), stack(g, "seen"), **PARAMS)
        oc.landmarks_build_carried(ctx, K, stack(g, "tracks"), stack(g, "seen"))
        if with_priors:
            op.landmarks_priors_carried(ctx, WEIGHT)
            op.bundle_adjust_landmarks_prior(ctx, start=START_ANCHOR)
        else:
            ctx.bundle_adjust_landmarks()
        results.append(oc.window_poses_pnp_carried_fetch(ctx))
        assert (ctx.landmarks_fetch()["status"] == L.OK).all()
        _, ss, sx = ctx.bundle_adjust_landmarks_fetch()
        assert any(s["termination"] == B.CONVERGENCE for s in ss), ss
        if with_priors:
            pri = op.landmarks_priors_fetch(ctx)
            on = pri["prior_weight"] > 0
            assert on.sum() >= 30 * len(wins[g])
            A = pri["prior_xyz"][on]
            move = max(move, float(np.max(np.linalg.norm(sx[on] - A, axis=1) / np.linalg.norm(A, axis=1))))
    return R.scale_deviation(results, wins, 3.0)[0], move


def test_priors_keep_the_carried_landmarks_and_the_scale(pkg, ctx):
    """Three generations of two streams whose first map is 3 x too large.  With priors (weight 1, from the anchors)
    the anchored landmarks of generations 1 and 2 stay where they were carried from, and the length ratio of the
    localised windows deviates no more than with the plain solve on the same streams."""
    wins = R.scale_streams()
    plain, _ = scale_run(pkg, ctx, wins, False)
    prior, move = scale_run(pkg, ctx, wins, True)
    print("device: ratio plain %.6e, with priors %.6e; anchored landmarks moved by %.3e (relative)" % (plain, prior, move))
    assert prior <= plain
    assert move <= 10 * ANCHOR_MOVE_MEASURED and prior <= 10 * PRIOR_RATIO_MEASURED


# ---- 13. refusals write nothing ------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pkg, mixed):
    oc, op = pkg.orbx_carry, pkg.orbx_prior
    bad = pkg.orbx.ERR_INVALID_ARG

    def refused(f, *a, **kw):
        with pytest.raises(pkg.OrbxError) as e:
            f(*a, **kw)
        assert e.value.status == bad, (f.__name__, a[1:], kw)

    olds, news = [m[:2] for m in mixed]
    win = B.make_window(1700, 5, 40, sigma=0.3)
    anchors, weights = mixed_priors(win, 1701)
    weights[0] = 1.0
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8)) as ctx:
        refused(op.landmarks_priors_carried, ctx, WEIGHT)  # no landmarks block, no carry block
        refused(op.bundle_adjust_landmarks_prior, ctx)     # no priors block
        refused(op.landmarks_priors_fetch, ctx)
        poses, tracks, seen = R.stack_old(olds)
        ctx.landmarks_build(K, tracks, seen, poses)
        refused(op.landmarks_priors_carried, ctx, WEIGHT)  # still no carry block
        dev = device_generation(pkg, ctx, olds, news, START_ANCHOR)

        def unchanged():
            LS.assert_blocks_equal(ctx.landmarks_fetch(), dev["block"])
            pri = op.landmarks_priors_fetch(ctx)
            for k in ("prior_xyz", "prior_weight", "count"):
                assert pri[k].tobytes() == dev["priors"][k].tobytes(), k
            sp, ss, sx = ctx.bundle_adjust_landmarks_fetch()
            assert sp.tobytes() == dev["solve"][0].tobytes() and ss == dev["solve"][1]
            assert sx.tobytes() == dev["solve"][2].tobytes()

        for w in (-1.0, float("nan"), float("inf"), -0.5):
            refused(op.landmarks_priors_carried, ctx, w)
        for kw in (dict(start=2), dict(start=-1), dict(huber_delta=0.0), dict(max_iters=0), dict(max_iters=1001)):
            refused(op.bundle_adjust_landmarks_prior, ctx, **kw)
        unchanged()
        # the host entries: the new cases, each with every output left as it was given
        base = dict(K=B.K_KITTI, poses=win["poses0"], points=win["pts0"], obs_point=win["obs_point"],
                    obs_pose=win["obs_pose"], obs_xy=win["obs_xy"], prior_xyz=anchors, prior_weight=weights)
        neg, nan_w, inf_w, nan_a = weights.copy(), weights.copy(), weights.copy(), anchors.copy()
        neg[3], nan_w[3], inf_w[3], nan_a[0, 1] = -1.0, np.nan, np.inf, np.nan
        for name, kw in (("negative weight", dict(prior_weight=neg)), ("nan weight", dict(prior_weight=nan_w)),
                         ("infinite weight", dict(prior_weight=inf_w)), ("nan anchor", dict(prior_xyz=nan_a)),
                         ("start 2", dict(start=2)), ("no weights", dict(prior_weight=None)),
                         ("no anchors", dict(prior_xyz=None)), ("delta 0", dict(huber_delta=0.0)),
                         ("max_iters 0", dict(max_iters=0))):
            refused(op.bundle_adjust_prior, ctx, **{**base, **kw})
        # ... and a non-finite anchor under weight 0 is not an error
        free = nan_a.copy()
        lam0 = weights.copy()
        lam0[0] = 0.0
        assert same(op.bundle_adjust_prior(ctx, **{**base, "prior_xyz": free, "prior_weight": lam0}),
                    op.bundle_adjust_prior(ctx, **{**base, "prior_weight": lam0}))
        unchanged()
        # a carry block of another capacity: the gather is refused, the priors block stays
        origin, tracks, seen = R.stack_new(news)
        oc.landmarks_carry(ctx, origin[:, :100].copy())
        refused(op.landmarks_priors_carried, ctx, WEIGHT)
        unchanged()
        oc.landmarks_carry(ctx, origin)
        # priors gathered, the landmarks rebuilt: the solve with them is refused and nothing is written
        ctx.landmarks_build(K, tracks, seen, dev["pnp"]["poses6"])
        rebuilt = ctx.landmarks_fetch()
        refused(op.bundle_adjust_landmarks_prior, ctx, start=START_ANCHOR)
        LS.assert_blocks_equal(ctx.landmarks_fetch(), rebuilt)
        pri = op.landmarks_priors_fetch(ctx)
        for k in ("prior_xyz", "prior_weight", "count"):
            assert pri[k].tobytes() == dev["priors"][k].tobytes(), k
        with pytest.raises(pkg.OrbxError):  # (the rebuilt block has not been solved)
            ctx.bundle_adjust_landmarks_fetch()
        op.landmarks_priors_carried(ctx, WEIGHT)  # gathered again for the new block, the solve is taken
        op.bundle_adjust_landmarks_prior(ctx, start=START_ANCHOR)
        assert len(ctx.bundle_adjust_landmarks_fetch()[1]) == 2


# ---- 14. callers' streams --------------------------------------------------------------------------------------------------
def test_callers_streams(pkg, ctx, mixed):
    import torch

    olds, news = [m[:4] for m in mixed]
    ref = device_generation(pkg, ctx, olds, news, START_ANCHOR)
    device_generation(pkg, ctx, mixed[0][4:8], mixed[1][4:8], START_GIVEN, weight=7.0)  # other blocks in between
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = device_generation(pkg, ctx, olds, news, START_ANCHOR, gather_stream=s1.cuda_stream,
                            solve_stream=s2.cuda_stream)  # the carried build ran on the context's stream
    for k in ("prior_xyz", "prior_weight", "count"):
        assert got["priors"][k].tobytes() == ref["priors"][k].tobytes(), k
    assert got["solve"][0].tobytes() == ref["solve"][0].tobytes() and got["solve"][1] == ref["solve"][1]
    assert got["solve"][2].tobytes() == ref["solve"][2].tobytes()
    assert any(s["termination"] == B.CONVERGENCE for s in got["solve"][1])
    torch.cuda.synchronize()
