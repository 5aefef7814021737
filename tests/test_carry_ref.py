"""The numpy restatement of the landmarks carry (tests/carry_ref.py) checked without a GPU: on
clean streams its poses are the true ones, on the edge cases its statuses are as designed -- the condition that every
window of tests/test_carry.py's mixed batch is what it is there for -- and the chain of three generations keeps the
scale of its first map within the constants tests/test_carry.py allows ten times of."""
import numpy as np
import pytest

import carry_ref as R
import landmarks_ref as L
import landmarks_seq as LS
import pnp_ref as PR
import pnp_seq as S

PARAMS = R.MIX_PARAMS
# tests/test_carry.py: SCALE_RATIO_MEASURED, SCALE_ROT_MEASURED, FRAME0_ROT_MEASURED, FRAME0_T_MEASURED
MEASURED = (8.0e-7, 2.3e-8, 5.0e-8, 4.5e-6)


@pytest.fixture(scope="module")
def lm(tmp_path_factory):
    return LS.compile_so(tmp_path_factory.mktemp("lm_seq_carry"), "lm_sequential")


@pytest.fixture(scope="module")
def pnp(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("pnp_seq_carry"))


def block_of(lm, olds):
    poses, tracks, seen = R.stack_old(olds)
    return LS.seq_build(lm, R.K, poses, tracks, seen)


def test_join_by_hand():
    block = dict(status=np.array([L.OK, L.EMPTY, L.OK], np.int32), point_offset=np.array([0, 3, 3, 5], np.int32),
                 slot_of_point=np.array([1, 4, 6, 0, 5], np.int32),
                 points3=np.arange(15, dtype=np.float64).reshape(5, 3) + 1.0)
    block["points3"][4, 1] = np.inf
    origin = np.array([[4, 1, 6, 0, 7, -1, 4], [0, 1, 2, 3, 4, 5, 6], [0, 5, 1, 8, 0, -2, 9]], np.int32)
    c = R.join(block, origin, 8)
    assert c["point"].tolist() == [[1, 0, 2, -1, -1, -1, 1], [-1] * 7, [0, -1, -1, -1, 0, -1, -1]]
    assert c["count"].tolist() == [4, 0, 2]
    assert c["xyz"][0, 0].tolist() == [4.0, 5.0, 6.0] and c["xyz"][2, 4].tolist() == [10.0, 11.0, 12.0]
    assert not c["xyz"][1].any() and not c["xyz"][2, 1].any()  # a landmark that is not finite is not carried
    # an origin beyond the old capacity is not looked up, whatever slot_of_point holds
    assert R.join(block, origin, 6)["point"][0].tolist() == [1, 0, -1, -1, -1, -1, 1]
    # another source: the same join, other coordinates
    other = R.join(block, origin, 8, points=block["points3"] * 2.0)
    assert np.array_equal(other["point"][0], c["point"][0]) and np.array_equal(other["xyz"][0], 2.0 * c["xyz"][0])
    assert other["point"][2].tolist() == c["point"][2].tolist()


def test_gather_by_hand():
    carry = dict(point=np.array([[0, -1, 2, 3, 4]], np.int32), xyz=np.arange(15, dtype=np.float64).reshape(1, 5, 3))
    tracks = np.ones((1, 5, 3, 2), np.float32)
    tracks[0, 3, 1, 0] = np.nan
    tracks[0, 0, 2] = [0.1, 0.2]
    seen = np.array([[3, 3, 1, 7, -4]], np.int32)
    assert [R.gather(carry, tracks, seen, 0, k)[0].tolist() for k in range(3)] == [[0, 2, 3], [0], [0, 3]]
    _, X, px = R.gather(carry, tracks, seen, 0, 2)
    assert X.tolist() == [[0.0, 1.0, 2.0], [9.0, 10.0, 11.0]] and px.dtype == np.float64
    assert px[0].tolist() == [float(np.float32(0.1)), float(np.float32(0.2))]  # widened, not re-rounded


def test_fill_by_hand():
    rec = np.zeros((4, 4), S.RECORD)
    rec["pose6"] = np.arange(96, dtype=np.float64).reshape(4, 4, 6) + 1.0
    rec["status"][1, 1] = S.FEW_POINTS
    rec["status"][2, 0] = S.NO_MODEL
    rec["status"][3, 2:] = S.NO_MODEL
    poses, status = R.fill(rec)
    assert status.tolist() == [R.CARRY_OK, R.CARRY_LOST, R.CARRY_LOST, R.CARRY_OK]
    assert np.array_equal(poses[0], rec["pose6"][0]) and not poses[1].any() and not poses[2].any()
    assert np.array_equal(poses[3, :2], rec["pose6"][3, :2])
    assert np.array_equal(poses[3, 2], rec["pose6"][3, 1]) and np.array_equal(poses[3, 3], rec["pose6"][3, 1])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_on_a_clean_stream_the_poses_are_the_true_ones(lm, pnp, seed):
    _, old, new = R.two_generations(seed, W=4, old_slots=80, fresh=10, min_seen=0)
    block = LS.seq_build(lm, R.K, old["true_poses"][None], old["tracks"][None], old["seen"][None])
    carry = R.join(block, new["origin"][None], 80)
    alive = int((old["seen"] == 4).sum())
    assert block["status"][0] == L.OK and carry["count"][0] == alive and 5 < alive < 40
    assert (carry["point"][0, :alive] >= 0).all() and (carry["point"][0, alive:] == -1).all()
    ref = R.localise(pnp, carry, new["tracks"][None], new["seen"][None], **PARAMS)
    assert ref["window_status"][0] == R.CARRY_OK and (ref["records"]["status"] == S.OK).all()
    assert (ref["records"]["inliers"] == alive).all() and ref["mask"][0, :, :alive].all()
    assert not ref["mask"][0, :, alive:].any()
    for k in range(4):  # in the OLD window's frame: no scale ratio, no alignment
        er, et = PR.pose_error(ref["poses6"][0, k], L.rodrigues(new["true_poses"][k, :3]), new["true_poses"][k, 3:])
        assert er < 1e-4 and et < 1e-2, (k, er, et)
    assert ref["poses6"].tobytes() == ref["records"]["pose6"].tobytes()


def test_every_window_of_the_mixed_batch_is_what_it_is_there_for(lm, pnp):
    olds, news = R.mixed_batch()
    block = block_of(lm, olds)
    origin, tracks, seen = R.stack_new(news)
    carry = R.join(block, origin, R.MIX_CAP)
    ref = R.localise(pnp, carry, tracks, seen, **PARAMS)
    R.check_mixed(block, carry, ref, news)
    # the clean windows give the true poses
    for w in (0, 1, 2, 6, 7):
        for k in range(R.MIX_W):
            truth = news[w]["true_poses"][k]
            er, et = PR.pose_error(ref["poses6"][w, k], L.rodrigues(truth[:3]), truth[3:])
            assert er < 1e-4 and et < 1e-2, (w, k, er, et)


def test_a_window_does_not_depend_on_its_place_in_the_batch(lm, pnp):
    olds, news = R.mixed_batch()
    block = block_of(lm, olds)
    origin, tracks, seen = R.stack_new(news)
    whole = R.localise(pnp, R.join(block, origin, R.MIX_CAP), tracks, seen, **PARAMS)
    one = block_of(lm, olds[1:2])
    alone = R.localise(pnp, R.join(one, origin[1:2], R.MIX_CAP), tracks[1:2], seen[1:2], **PARAMS)
    assert alone["records"].tobytes() == whole["records"][1:2].tobytes()
    assert alone["mask"].tobytes() == whole["mask"][1:2].tobytes()


def test_three_generations_keep_the_scale_of_the_first_map(lm, pnp):
    """the measurement tests/test_carry.py's bounds stand on"""
    wins = R.scale_streams()
    res = R.cpu_generations(lm, pnp, wins, 3.0, **PARAMS)
    got = R.scale_deviation(res, wins, 3.0)
    print("ratio %.3e, rotation %.3e rad, frame 0: %.3e rad, %.3e units" % got)
    assert all(g <= m for g, m in zip(got, MEASURED)), got
    assert all(g > m / 10 for g, m in zip(got, MEASURED)), got  # (the constants are the measurement, not a roof)
    # the chained scale really is the first map's: the same streams from a true first map give ratio 1, not 3
    true = R.scale_deviation(R.cpu_generations(lm, pnp, wins, 1.0, **PARAMS), wins, 1.0)
    assert true[0] < 1e-5
