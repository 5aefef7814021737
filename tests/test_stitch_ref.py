"""CPU tests of the join of overlapping windows into one trajectory (include/orbx_stream.h): the
host entry orbx_stitch_windows against

  seq     tests/cpp/st_sequential.cpp, the sequential restatement on the same arithmetic: bit for bit
  numpy   tests/stitch_ref.py in longdouble, within stitch_ref.tolerance -- whose constant this file measures
  truth   the true path of the generator's streams, within the same bound (gauge recovery)

and the rules one by one: the owner table, broken windows, degenerate baselines, refusals.  No GPU is touched."""
import numpy as np
import pytest

import stitch_ref as R
import stitch_seq as SS

CASES = {cs["name"]: cs for cs in R.cases()}


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return SS.compile_seq(tmp_path_factory.mktemp("st_seq"))


@pytest.fixture(scope="module")
def S(pkg):
    return pkg.orbx_stream


@pytest.fixture(scope="module")
def routes():
    """every case through the numpy restatement, once: name -> (float64 result, longdouble result)"""
    return {name: tuple(R.stitch(cs["poses"], cs["stride"], cs["T_start"], cs["align_scale"], dt)
                        for dt in (np.float64, np.longdouble)) for name, cs in CASES.items()}


def test_the_cases_are_the_shapes_and_gauges_they_claim():
    shapes = {(cs["poses"].shape[0], cs["poses"].shape[1], cs["stride"]) for cs in CASES.values()}
    assert shapes == set(R.SHAPES)
    scaled = [cs for cs in CASES.values() if cs["scaled"]]
    assert {(cs["poses"].shape[0], cs["poses"].shape[1], cs["stride"]) for cs in scaled} == \
        {(W, L, s) for W, L, s in R.SHAPES if s <= L - 2}  # where rule 3 allows the alignment
    for cs in scaled:
        g = cs["gauge_scale"]
        assert g[0] == 1.0 and g[1:].min() >= 0.3 and g[1:].max() <= 3.0 and (g[1:] != 1.0).all()
    assert max(np.abs(cs["true"][:, :3, 3].astype(np.float64)).max() for cs in CASES.values()) > 100.0


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_entry_equals_the_sequential_restatement(S, seq, name, given):
    cs = CASES[name]
    T = cs["T_start"] if given else None
    for align in ((False, True) if cs["stride"] <= cs["poses"].shape[1] - 2 else (False,)):
        got = S.stitch_windows(cs["poses"], cs["stride"], T, align)
        SS.assert_stitch_equal(got, SS.seq_stitch(seq, cs["poses"], cs["stride"], T, align))
        assert (got["trajectory4x4"][:, 3] == [0.0, 0.0, 0.0, 1.0]).all()
        if not align:
            assert (got["lambda"] == 1.0).all()
        assert (got["status"] == R.OK).all()


def test_the_tolerance_is_what_stitch_ref_says(routes):
    """measures the float64 numpy route against the longdouble one on cases(): stitch_ref.TOLERANCE_REL is 16 x the
    largest scaled distance, and what is measured here is not above the value written there"""
    worst = 0.0
    for name, (f64, ld) in routes.items():
        d, sc = R.distance(f64, ld), R.scale(CASES[name], ld)
        print("%-22s scale %7.1f  float64 - longdouble %.3e  scaled %.3e" % (name, sc, d, d / sc))
        worst = max(worst, d / sc)
    print("largest scaled distance %.3e, TOLERANCE_REL %.3e" % (worst, R.TOLERANCE_REL))
    assert 0.0 < worst <= R.TOLERANCE_REL / 16


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_entry_against_numpy_in_longdouble(S, routes, name):
    cs, ld = CASES[name], routes[name][1]
    got = S.stitch_windows(cs["poses"], cs["stride"], cs["T_start"], cs["align_scale"])
    d, tol = R.distance(got, ld), R.tolerance(cs, ld)
    print("%s: distance %.3e, tolerance %.3e" % (name, d, tol))
    assert d <= tol
    assert np.array_equal(got["owner"], ld["owner"]) and np.array_equal(got["status"], ld["status"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_gauge_recovery(S, routes, name):
    """the stitched trajectory is the true one, whatever rigid motion -- and, with align_scale, whatever scale --
    each window came in"""
    cs, ld = CASES[name], routes[name][1]
    got = S.stitch_windows(cs["poses"], cs["stride"], cs["T_start"], cs["align_scale"])
    d = float(np.max(np.abs(got["trajectory4x4"].astype(np.longdouble) - cs["true"])))
    tol = R.tolerance(cs, ld)
    print("%s: distance to the true path %.3e, tolerance %.3e" % (name, d, tol))
    assert d <= tol
    if cs["scaled"]:
        want = 1.0 / cs["gauge_scale"]
        assert np.max(np.abs(got["lambda"] - want) / want) <= R.TOLERANCE_REL * max(1.0, R.scale(cs, ld))
        # without the alignment the scaled windows do not join
        off = S.stitch_windows(cs["poses"], cs["stride"], cs["T_start"], False)
        assert np.max(np.abs(off["trajectory4x4"].astype(np.longdouble) - cs["true"])) > 1e3 * tol


@pytest.mark.parametrize("shape", R.SHAPES)
def test_owner_table_and_first_pose(S, shape):
    W, L, stride = shape
    rng = np.random.default_rng(W * 100 + L * 10 + stride)
    cs = R.make_stream(W, L, stride, 900, False)
    poses = cs["poses"].copy()
    # window 0 in the gauge where its first pose is the identity, as it comes out of its chain
    inv0 = np.linalg.inv(poses[0, 0])
    poses[0] = inv0 @ poses[0]
    poses[0, 0] = np.eye(4)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.WR.rot(rng.normal(size=3), 0.9), rng.normal(size=3) * 7.0
    got = S.stitch_windows(poses, stride, T)
    own, idx = R.owner_table(W, L, stride)
    assert np.array_equal(got["owner"], own) and len(own) == (W - 1) * stride + L
    for w in range(W):  # window w contributes its frames 0 .. stride - 1, the last one all L
        assert idx[own == w].tolist() == list(range(L if w == W - 1 else stride))
    assert SS.bits_equal(got["trajectory4x4"][0], T) and SS.bits_equal(got["anchors4x4"][0], T)
    # without a T_start the stream starts at the identity
    assert SS.bits_equal(S.stitch_windows(poses, stride)["trajectory4x4"][0], np.eye(4))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_broken_window_stands_still(S, seq, bad):
    cs = CASES["W5_L5_s2_scaled"]
    stride, T = cs["stride"], cs["T_start"]
    poses = cs["poses"].copy()
    poses[2, 4, 1, 2] = bad  # a frame window 2 does not even own
    good = S.stitch_windows(cs["poses"], stride, T, True)
    got = S.stitch_windows(poses, stride, T, True)
    SS.assert_stitch_equal(got, SS.seq_stitch(seq, poses, stride, T, True))
    ref = R.stitch(poses, stride, T, True)
    assert got["status"].tolist() == ref["status"].tolist() == [R.OK, R.OK, R.BROKEN, R.SCALE_UNALIGNED, R.OK]
    assert np.isfinite(got["trajectory4x4"]).all() and np.isfinite(got["anchors4x4"]).all()
    first = 2 * stride  # the frames before the window are untouched
    assert SS.bits_equal(got["trajectory4x4"][:first], good["trajectory4x4"][:first])
    assert SS.bits_equal(got["anchors4x4"][:3], good["anchors4x4"][:3])
    owned = got["owner"] == 2
    assert owned.sum() == stride and all(SS.bits_equal(T4, got["anchors4x4"][2]) for T4 in got["trajectory4x4"][owned])
    assert SS.bits_equal(got["anchors4x4"][3], got["anchors4x4"][2])
    # lambda: the broken window keeps the factor it arrived with, the one behind it is not aligned to it
    assert got["lambda"][2] == got["lambda"][1] == got["lambda"][3]
    assert R.distance(got, ref) <= R.tolerance(cs, ref)


def test_equal_camera_centres_leave_the_scale_unaligned(S, seq):
    cs = CASES["W5_L5_s2_scaled"]
    stride, T = cs["stride"], cs["T_start"]
    for w, (a, b), hit in ((3, (0, 1), 3), (1, (stride, stride + 1), 2)):  # b_first(3) = 0; b_link(1) = 0
        poses = cs["poses"].copy()
        poses[w, b, :3, 3] = poses[w, a, :3, 3]
        got = S.stitch_windows(poses, stride, T, True)
        SS.assert_stitch_equal(got, SS.seq_stitch(seq, poses, stride, T, True))
        want = [R.OK] * 5
        want[hit] = R.SCALE_UNALIGNED
        assert got["status"].tolist() == want == R.stitch(poses, stride, T, True)["status"].tolist()
        assert got["lambda"][hit] == got["lambda"][hit - 1]  # lambda(hit) = 1
        assert (S.stitch_windows(poses, stride, T, False)["status"] == R.OK).all()


def test_refusals(pkg, S):
    P = np.tile(np.eye(4), (3, 4, 1, 1))
    bad_T = np.eye(4)
    bad_T[1, 3] = np.nan
    for args in ((P, 0), (P, 4), (P, 3, None, True), (P, 2, bad_T), (P[:, :1], 1), (P[:0], 1)):
        with pytest.raises(pkg.OrbxError) as e:
            S.stitch_windows(*args)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
    lib = S.load()
    assert lib.orbx_stitch_windows(None, 3, 4, 1, None, 0, None, None, None, None, None) == pkg.orbx.ERR_INVALID_ARG
    # every output may be NULL
    assert lib.orbx_stitch_windows(P.ctypes.data, 3, 4, 3, None, 0, None, None, None, None, None) == pkg.orbx.OK
    S.stitch_windows(P, 3)  # stride == L - 1 without the alignment
