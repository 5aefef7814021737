"""ORB descriptors at caller-held points and the re-association by descriptor on the device (DESIGN.md §9 rank 19;
include/orbx_reloc.h).  state, n_ok, the descriptor bytes and the angle BITS are compared with tests/reassoc_ref.py's
restatement of rules A-E on the CPU oracle; origin, dist and count with its restatement of rules F-J; everything for
equality.  The first cases are small: 96 slots (no multiple of the classify workgroup's 256, 24 describe workgroups of
which most leave early), a frame smaller than the context's maximum, one with a row stride above its width, 300 train
slots (two LDS tiles, the second one partial).  They are below the sizes at which k_pd_classify carries its base from
one chunk of 256 slots into the next, k_ra_knn2 has a second workgroup per window and k_ra_unique a second chunk, and
their widths are multiples of 4; the cases of 513 slots on 67 x 50 and 130 x 47 frames and of 513 x 256 and 257 x 513
descriptor sets are there for those."""
import numpy as np
import pytest

import carry_ref as CR
import reassoc_ref as R
import test_reloc_shift_ref as SH

pytestmark = pytest.mark.gpu
W, H, CAP = 320, 160, 96


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def crop(oracle):
    return oracle.load_kitti(0)[100:260, 300:620].copy()


def case_points(w, h, rng, r=20):
    """CAP points for a w x h frame: the ties of both parities, every border at r and r - 1, what is not usable, then
    random interior floats"""
    fixed = [(20.5, 20.0), (21.5, 20.0), (20.0, 20.5), (20.0, 21.5), (22.5, 23.5),            # .5 ties, both parities
             (r, r), (r - 1, r), (r, r - 1), (w - 1 - r, h - 1 - r), (w - r, h - 1 - r), (w - 1 - r, h - r),
             (w - 1 - r, r), (r, h - 1 - r), (w - 1 - r + 0.49, 50.0), (w - 1 - r + 0.5, 50.0), (w - 1 - r + 0.51, 50.0),
             (r - 0.5, 60.0), (r - 0.51, 60.0), (60.0, h - 1 - r + 0.5), (60.0, h - 1 - r + 0.51),
             (np.nan, 50.0), (50.0, np.nan), (np.inf, 50.0), (50.0, -np.inf), (-1.0, 50.0), (50.0, -0.25),
             (w - 1.0, h - 1.0), (w - 0.99, 50.0), (50.0, h - 0.5), (1e9, 50.0), (0.0, 0.0), (-0.0, 30.0)]
    pts = np.zeros((CAP, 2), np.float32)
    pts[:len(fixed)] = fixed
    n = CAP - len(fixed)
    pts[len(fixed):] = np.c_[rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)]
    return pts


@pytest.fixture(scope="module")
def case(crop):
    """three frames: the crop, the crop inside a pitch of 352, the 312 x 152 corner of the crop; the points sit in an
    array shaped like an LK view of five frames (point_stride 10), in its frame 3"""
    rng = np.random.default_rng(19)
    sizes = [(W, H), (W, H), (312, 152)]
    imgs = [crop, crop[::-1].copy(), crop[:152, :312].copy()]
    pts = np.stack([case_points(w, h, rng) for w, h in sizes])
    seen = np.full((3, CAP), 5, np.int32)
    seen[:, 40:48] = rng.integers(0, 4, (3, 8))  # gated by seen_min = 4
    seen[1, 0] = 3
    counts = np.array([CAP, CAP, 90], np.int32)
    return dict(sizes=sizes, imgs=imgs, pts=pts, seen=seen, counts=counts)


def reference(oracle, case, blur_levels, blur_kind=0):
    p = oracle.gpu_params(blur_levels=blur_levels, blur_kind=blur_kind)
    return [R.describe_points(case["imgs"][f], case["pts"][f], p, seen=case["seen"][f], seen_min=4,
                              count=int(case["counts"][f])) for f in range(3)]


def upload(case):
    """(frames of the first two (2, H, 352)[:, :, :W] -- a row stride above the width --, the third frame, the LK-shaped
    track block, seen, counts) on the device"""
    import torch

    two = np.zeros((2, H, 352), np.uint8)
    two[:] = 255  # (what lies between the width and the row stride is not the image)
    two[0, :, :W], two[1, :, :W] = case["imgs"][0], case["imgs"][1]
    tracks = np.full((3, CAP, 5, 2), -7.0, np.float32)
    tracks[:, :, 3] = case["pts"]
    out = [torch.from_numpy(a).cuda() for a in (two, case["imgs"][2], tracks, case["seen"], case["counts"])]
    torch.cuda.synchronize()
    return out


def run_describe(pkg, ctx, dev, bank=0):
    """frames 0 and 1 in one call (strided rows), frame 2 (smaller than max) in another; returns the three frames"""
    two, small, tracks, seen, counts = dev
    o = pkg.orbx_reloc
    o.describe_points(ctx, two[:, :, :W], tracks[:2, :, 3], bank=bank, seen=seen[:2].contiguous(), seen_min=4,
                      counts=counts[:2].contiguous())
    a = o.point_descriptors_fetch(ctx, bank)
    o.describe_points(ctx, small[None], tracks[2:, :, 3], bank=bank, seen=seen[2:].contiguous(), seen_min=4,
                      counts=counts[2:].contiguous())
    b = o.point_descriptors_fetch(ctx, bank)
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def assert_described(got, ref):
    for f in range(3):
        r = ref[f]
        assert got["state"][f].tolist() == r["state"].tolist(), f
        assert got["n_ok"][f] == r["n_ok"] == (r["state"] == R.PD_OK).sum(), f
        assert got["desc"][f].tobytes() == r["desc"].tobytes(), f
        assert np.array_equal(bits(got["angle"][f]), bits(r["angle"])), f
        dead = r["state"] != R.PD_OK
        assert not got["desc"][f][dead].any() and not bits(got["angle"][f])[dead].any()


@pytest.mark.parametrize("blur_levels,blur_kind", [(0, 0), (2, 0), (2, 1)])
def test_describe_parity(pkg, oracle, case, blur_levels, blur_kind):
    ref = reference(oracle, case, blur_levels, blur_kind)
    # the case is what it is there for: every state occurs, the ties round to even, the gates bite
    st = np.stack([r["state"] for r in ref])
    assert all((st[f] == s).sum() >= 8 for f in range(3) for s in (R.PD_NONE, R.PD_BORDER, R.PD_OK))
    assert ref[0]["pix"][:5].tolist() == [[20, 20], [22, 20], [20, 20], [20, 22], [22, 24]]
    assert st[0, :9].tolist() == [R.PD_OK] * 6 + [R.PD_BORDER] * 2 + [R.PD_OK] and st[0, 9] == R.PD_BORDER
    assert st[0, 13:18].tolist() == [R.PD_OK, R.PD_BORDER, R.PD_BORDER, R.PD_OK, R.PD_BORDER]  # 299.5 -> 300, 19.5 -> 20
    assert (st[:, 40:48] == R.PD_NONE).sum() >= 20 and st[1, 0] == R.PD_NONE and (st[2, 90:] == R.PD_NONE).all()
    assert all(r["nskip"] == 0 and r["noob"] == 0 for r in ref)
    dev = upload(case)
    params = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=4, blur_levels=blur_levels,
                                blur_kind=blur_kind)
    with pkg.Context(params) as ctx:
        o = pkg.orbx_reloc
        got = run_describe(pkg, ctx, dev)
        assert_described(got, ref)
        v = o.point_descriptors_view(ctx, 0)
        assert (v.n, v.slot_capacity) == (1, CAP) and v.desc and v.angle and v.state and v.n_ok
        # a call to bank 1 leaves bank 0's fetched bytes unchanged
        bank0 = o.point_descriptors_fetch(ctx, 0)
        two, small, tracks, seen, counts = dev
        o.describe_points(ctx, two[:, :, :W], tracks[:2, :, 3], bank=1)
        again = o.point_descriptors_fetch(ctx, 0)
        assert all(again[k].tobytes() == bank0[k].tobytes() for k in bank0)
        full = o.point_descriptors_fetch(ctx, 1)
        assert full["n_ok"].sum() > got["n_ok"][:2].sum()  # (no seen gate, no counts)
        assert o.point_descriptors_fetch(ctx, 1, 1, 1)["desc"].tobytes() == full["desc"][1:].tobytes()
        # a workspace bound below two frames: one frame per slice, the same arrays
        o.describe_points_workspace_limit(ctx, 64 * 1024)
        assert_described(run_describe(pkg, ctx, dev), ref)
        o.describe_points(ctx, two[:, :, :W], tracks[:2, :, 3], bank=1)
        sliced = o.point_descriptors_fetch(ctx, 1)
        assert all(sliced[k].tobytes() == full[k].tobytes() for k in full)
        o.describe_points_workspace_limit(ctx, 0)
        # the host entry: frame 2's points on its image, as a batch of one frame in bank 0
        one = o.describe_points_host(ctx, case["imgs"][2], case["pts"][2])
        plain = R.describe_points(case["imgs"][2], case["pts"][2],
                                  oracle.gpu_params(blur_levels=blur_levels, blur_kind=blur_kind))
        assert one["state"].tolist() == plain["state"].tolist() and one["desc"].tobytes() == plain["desc"].tobytes()
        assert np.array_equal(bits(one["angle"]), bits(plain["angle"]))
        assert o.point_descriptors_view(ctx, 0).slot_capacity == CAP and o.point_descriptors_view(ctx, 0).n == 1


BIG = 513  # beyond two chunks of the classify workgroup: its base is carried twice, the third chunk is partial


def big_points(w, h, rng, r=20):
    """BIG points for a w x h frame: case_points' fixed ones, then three random floats inside rule C's interior for
    every one anywhere in the frame -- OK slots in every chunk of 256, with other states between them"""
    pts = np.zeros((BIG, 2), np.float32)
    pts[:CAP] = case_points(w, h, rng, r)
    n = BIG - CAP
    inside = np.c_[rng.uniform(r - 0.5, w - 1 - r + 0.5, n), rng.uniform(r - 0.5, h - 1 - r + 0.5, n)]
    anywhere = np.c_[rng.uniform(-1, w, n), rng.uniform(-1, h, n)]
    pts[CAP:] = np.where((np.arange(n) % 4 < 3)[:, None], inside, anywhere)
    return pts


@pytest.mark.parametrize("blur_levels,blur_kind", [(0, 0), (2, 0), (2, 1)])
def test_describe_parity_on_narrow_frames_of_many_slots(pkg, oracle, blur_levels, blur_kind):
    """67 x 50 and 130 x 47: widths that are no multiple of 4 (the last dword of a level-0 row is partial: the pixels
    inside the width are what is checked here -- the zeros k_pd_level0 writes from the width to the pitch are read by no
    OK slot, 20 pixels from every border, and no entry fetches the level-0 image), one of them a single tile of 64 and three more pixels, rows that start at
    every byte offset; 513 slots each"""
    import torch

    rng = np.random.default_rng(23)
    p = oracle.gpu_params(blur_levels=blur_levels, blur_kind=blur_kind)
    params = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=4, blur_levels=blur_levels,
                                blur_kind=blur_kind)
    with pkg.Context(params) as ctx:
        for (w, h), pitch in (((67, 50), 67), ((130, 47), 141)):
            imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
            imgs[1] = np.clip(np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256 + rng.integers(0, 9, (h, w)), 0, 255)
            pts = np.stack([big_points(w, h, rng) for _ in range(2)])
            counts = np.array([BIG, 400], np.int32)
            ref = [R.describe_points(imgs[f], pts[f], p, count=int(counts[f])) for f in range(2)]
            st = np.stack([r["state"] for r in ref])
            assert ref[0]["n_ok"] > 256 and ref[1]["n_ok"] > 200
            for lo in (0, 256):  # OK slots in every chunk, and others among them
                assert (st[0, lo:lo + 256] == R.PD_OK).any() and (st[0, lo:lo + 256] != R.PD_OK).any()
            assert st[0, 512] == R.PD_OK and (st[1, 400:] == R.PD_NONE).all()
            assert all((st[f] == s).sum() >= 8 for f in range(2) for s in (R.PD_NONE, R.PD_BORDER, R.PD_OK))
            parent = np.full((2, h, pitch), 255, np.uint8)  # (what lies between the width and the row stride is not the image)
            parent[:, :, :w] = imgs
            frames = torch.from_numpy(parent).cuda()[:, :, :w]
            torch.cuda.synchronize()
            o = pkg.orbx_reloc
            o.describe_points(ctx, frames, pts, counts=counts)
            got = o.point_descriptors_fetch(ctx, 0)
            for f in range(2):
                r = ref[f]
                assert got["state"][f].tolist() == r["state"].tolist(), (w, f)
                assert got["n_ok"][f] == r["n_ok"], (w, f)
                assert got["desc"][f].tobytes() == r["desc"].tobytes(), (w, f)
                assert np.array_equal(bits(got["angle"][f]), bits(r["angle"])), (w, f)


@pytest.mark.parametrize("blur_levels,interior", [(0, 37), (2, 82)])  # (counted on the CPU oracle)
def test_agreement_with_the_orb_path(pkg, crop, blur_levels, interior):
    """the interior level-0 keypoints of detect_and_compute, given back as float points, yield the angle bits and the
    descriptor bytes the ORB result holds for them"""
    params = pkg.default_params("gpu", nfeatures=300, nlevels=4, max_width=W, max_height=H, blur_levels=blur_levels)
    with pkg.Context(params) as ctx:
        orb = ctx.detect_and_compute(crop)
        kps = orb["kps"][:orb["count"]]
        pick = np.flatnonzero((orb["levels"][:orb["count"]] == 0) & (kps[:, 0] >= 20) & (kps[:, 0] <= W - 21) &
                              (kps[:, 1] >= 20) & (kps[:, 1] <= H - 21))
        assert len(pick) == interior
        got = pkg.orbx_reloc.describe_points_host(ctx, crop, kps[pick].astype(np.float32))
        assert (got["state"] == R.PD_OK).all()
        assert got["desc"].tobytes() == orb["desc"][pick].tobytes()
        assert np.array_equal(bits(got["angle"]), bits(orb["angles"][pick]))


@pytest.fixture(scope="module")
def sets():
    return R.synthetic_windows(70, 300)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=W, max_height=H, max_batch=8, blur_levels=SH.BLUR_LEVELS)) as c:
        yield c


@pytest.mark.parametrize("unique", [0, 1])
@pytest.mark.parametrize("ratio,max_distance", [(0.8, 40), (0.8, 256), (1.0, 40), (1.0, 256)])
def test_reassociation_parity(pkg, ctx, sets, unique, ratio, max_distance):
    qdesc, qstate, tdesc, tstate = sets
    ref = R.reassociate(qdesc, qstate, tdesc, tstate, ratio, max_distance, unique)
    assert ref["count"][0] > 15 and ref["count"].tolist()[1:] == [0, 0]
    o = pkg.orbx_reloc
    o.reassociate(ctx, qdesc, qstate, tdesc, tstate, ratio=ratio, max_distance=max_distance, unique=unique)
    got = o.reassociate_fetch(ctx)
    for k in ("origin", "dist", "count"):
        assert got[k].dtype == np.int32 and got[k].tobytes() == ref[k].tobytes(), k
    v = o.reassociate_view(ctx)
    assert (v.n_windows, v.q_capacity, v.t_capacity) == (3, 70, 300) and v.origin and v.dist and v.count
    assert o.reassociate_fetch(ctx, 1, 2)["origin"].tobytes() == ref["origin"][1:].tobytes()
    # one window on host arrays: the same rules, the block replaced by a batch of one
    one = o.reassociate_host(ctx, qdesc[0], qstate[0], tdesc[0], tstate[0], ratio, max_distance, unique)
    assert one["origin"].tobytes() == ref["origin"][0].tobytes() and one["dist"].tobytes() == ref["dist"][0].tobytes()
    assert one["count"] == ref["count"][0] and o.reassociate_view(ctx).n_windows == 1
    none = o.reassociate_host(ctx, qdesc[0], qstate[0], tdesc[0][:0], tstate[0][:0], ratio, max_distance, unique)
    assert (none["origin"] == -1).all() and (none["dist"] == -1).all() and none["count"] == 0
    assert o.reassociate_host(ctx, qdesc[0][:0], qstate[0][:0], tdesc[0], tstate[0])["count"] == 0


@pytest.mark.parametrize("qcap,tcap", [(513, 256), (257, 513)])
def test_reassociation_parity_beyond_one_workgroup_of_queries(pkg, ctx, qcap, tcap):
    """More than 256 query slots: k_ra_knn2 runs two or three workgroups per window, whose queries lower one train
    slot's key from different workgroups, and k_ra_unique walks its chunks more than once; 256 and 513 train slots: a
    train set of one full LDS tile, and of two and one slot."""
    rng = np.random.default_rng(31)
    sets = [R.pool_window(rng, qcap, tcap) for _ in range(2)]
    qdesc, tdesc = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    qstate, tstate = np.full((2, qcap), R.PD_OK, np.int32), np.full((2, tcap), R.PD_OK, np.int32)
    qstate[1, ::7], tstate[1, 5::11] = R.PD_BORDER, R.PD_NONE
    # the first query of the second workgroup: a copy of the first query that is accepted at distance 0
    before = R.reassociate(qdesc, qstate, tdesc, tstate, 0.8, 256, 0)
    for w in range(2):
        qdesc[w, 256] = qdesc[w, np.flatnonzero(before["dist"][w, :256] == 0)[0]]
    plain = R.reassociate(qdesc, qstate, tdesc, tstate, 0.8, 256, 0)
    uniq = R.reassociate(qdesc, qstate, tdesc, tstate, 0.8, 256, 1)
    # the sets are what they are there for: accepted queries in every block of 256, train slots that queries of
    # different blocks tie for at one distance, and one that the nearer query of another block takes
    tie = nearer = False
    for w in range(2):
        o, d = plain["origin"][w], plain["dist"][w]
        assert all((o[lo:lo + 256] >= 0).any() for lo in range(0, qcap, 256))
        for t in np.unique(o[o >= 0]):
            qs = np.flatnonzero(o == t)
            nearest = qs[d[qs] == d[qs].min()]
            tie = tie or len(set((nearest // 256).tolist())) > 1
            nearer = nearer or (d[qs[0]] > d[qs].min() and nearest[0] // 256 != qs[0] // 256)
    assert tie and (nearer or qcap == 257)  # (257: the second workgroup's one live query is the copy made above)
    assert (uniq["count"] < plain["count"]).all() and (uniq["count"] > 20).all()
    o = pkg.orbx_reloc
    for unique, ref in ((0, plain), (1, uniq)):
        o.reassociate(ctx, qdesc, qstate, tdesc, tstate, ratio=0.8, max_distance=256, unique=unique)
        got = o.reassociate_fetch(ctx)
        for k in ("origin", "dist", "count"):
            assert got[k].dtype == np.int32 and got[k].tobytes() == ref[k].tobytes(), (unique, k)
        one = o.reassociate_host(ctx, qdesc[1], qstate[1], tdesc[1], tstate[1], 0.8, 256, unique)
        assert one["origin"].tobytes() == ref["origin"][1].tobytes() and one["count"] == ref["count"][1]


def test_the_shifted_crops_end_to_end_on_the_device(pkg, ctx):
    """good features -> descriptors into banks 0 and 1 -> re-association, nothing fetched in between; origin equals
    the CPU reference of tests/test_reloc_shift_ref.py element for element"""
    import torch

    ref = SH.reference()
    o = pkg.orbx_reloc
    for bank, img in enumerate(ref["crops"]):
        frame = torch.from_numpy(img).cuda()[None]
        torch.cuda.synchronize()
        ctx.good_features_batch(frame, SH.MAX_CORNERS, SH.QUALITY, SH.MIN_DISTANCE)
        gv = ctx.good_features_view()
        o.describe_points(ctx, frame, gv.corners_xy, bank=bank, counts=gv.counts, slot_capacity=gv.slot_capacity,
                          point_stride=2, frame_stride=2 * gv.slot_capacity)
    train, query = o.point_descriptors_view(ctx, 0), o.point_descriptors_view(ctx, 1)
    o.reassociate(ctx, query, train_desc=train, ratio=SH.RATIO, max_distance=SH.MAX_DISTANCE, unique=SH.UNIQUE)
    got = o.reassociate_fetch(ctx)
    assert got["origin"][0].tolist() == ref["origin"].tolist()
    assert got["dist"][0].tolist() == ref["dist"].tolist() and got["count"][0] == ref["count"] >= SH.RIGHT_AT_LEAST
    for bank in (0, 1):
        d = o.point_descriptors_fetch(ctx, bank)
        assert d["state"][0].tolist() == ref["described"][bank]["state"].tolist()
        assert d["desc"][0].tobytes() == ref["described"][bank]["desc"].tobytes()


def test_callers_streams(pkg, ctx):
    """good features on one stream, the descriptors on a second, the re-association on a third and the carry on a
    fourth, with no synchronisation in between: every call waits on the device for the block it reads"""
    import torch

    ref = SH.reference()
    o = pkg.orbx_reloc
    olds = [CR.two_generations(950, 5, 24, 0, min_seen=5)[1]]
    ctx.landmarks_build(CR.K, olds[0]["tracks"][None], olds[0]["seen"][None], olds[0]["true_poses"][None])
    block = ctx.landmarks_fetch()
    frames = [torch.from_numpy(img).cuda()[None] for img in ref["crops"]]
    torch.cuda.synchronize()
    s = [torch.cuda.Stream() for _ in range(4)]
    for bank in (0, 1):
        s[0].wait_stream(s[1])  # (the caller's part: the next good-features batch replaces the view bank 0 reads)
        ctx.good_features_batch(frames[bank], SH.MAX_CORNERS, SH.QUALITY, SH.MIN_DISTANCE, stream=s[0].cuda_stream)
        gv = ctx.good_features_view()
        o.describe_points(ctx, frames[bank], gv.corners_xy, bank=bank, counts=gv.counts, slot_capacity=gv.slot_capacity,
                          point_stride=2, frame_stride=2 * gv.slot_capacity, stream=s[1].cuda_stream)
    o.reassociate(ctx, o.point_descriptors_view(ctx, 1), train_desc=o.point_descriptors_view(ctx, 0), ratio=SH.RATIO,
                  max_distance=SH.MAX_DISTANCE, unique=SH.UNIQUE, stream=s[2].cuda_stream)
    v = o.reassociate_view(ctx)
    pkg.orbx_carry.landmarks_carry(ctx, v.origin, n_windows=1, slot_capacity=v.q_capacity, stream=s[3].cuda_stream)
    got = pkg.orbx_carry.landmarks_carry_fetch(ctx)
    assert o.reassociate_fetch(ctx)["origin"][0].tolist() == ref["origin"].tolist()
    want = CR.join(block, ref["origin"][None], 24)
    assert want["count"][0] > 0  # (some matched train slots are below 24 and own a landmark)
    for k in ("point", "xyz", "count"):
        assert got[k].tobytes() == want[k].tobytes(), k
    torch.cuda.synchronize()


def test_into_the_carry(pkg, ctx):
    """view.origin of a re-association over uploaded descriptors is what the carry takes as d_origin"""
    W5, slots, qcap = 5, 24, 30
    olds = [CR.two_generations(900 + w, W5, slots, 0, min_seen=W5)[1] for w in range(2)]
    ctx.landmarks_build(CR.K, np.stack([o["tracks"] for o in olds]), np.stack([o["seen"] for o in olds]),
                        np.stack([o["true_poses"] for o in olds]))
    block = ctx.landmarks_fetch()
    assert (block["status"] == 0).all() and block["point_offset"][-1] >= 40
    rng = np.random.default_rng(77)
    tdesc = rng.integers(0, 256, (2, slots, 32), dtype=np.uint8)
    tstate = np.full((2, slots), R.PD_OK, np.int32)
    tstate[1, 5] = R.PD_BORDER
    qdesc = rng.integers(0, 256, (2, qcap, 32), dtype=np.uint8)
    qstate = np.full((2, qcap), R.PD_OK, np.int32)
    for w in range(2):
        for q, t in enumerate(rng.permutation(slots)[:20]):
            qdesc[w, q + 3] = R.flip(tdesc[w, t], rng, int(rng.integers(0, 30)))
    o = pkg.orbx_reloc
    o.reassociate(ctx, qdesc, qstate, tdesc, tstate, ratio=0.8, max_distance=64, unique=1)
    v = o.reassociate_view(ctx)
    pkg.orbx_carry.landmarks_carry(ctx, v.origin, n_windows=v.n_windows, slot_capacity=v.q_capacity)
    origin = o.reassociate_fetch(ctx)["origin"]
    assert origin.tobytes() == R.reassociate(qdesc, qstate, tdesc, tstate, 0.8, 64, 1)["origin"].tobytes()
    got, ref = pkg.orbx_carry.landmarks_carry_fetch(ctx), CR.join(block, origin, slots)
    assert (ref["count"] >= 15).all() and (ref["point"][:, :3] == -1).all()
    for k in ("point", "xyz", "count"):
        assert got[k].tobytes() == ref[k].tobytes(), k
