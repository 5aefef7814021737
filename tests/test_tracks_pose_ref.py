"""CPU tests of the tracks-pose restatement (tests/tracks_pose_ref.py): rule 1 on hand-built
`seen` tables, the invariants of the join on the slot, recovery of known motion, and the classes the GPU tests'
inputs contain."""
import numpy as np
import pytest

import landmarks_ref as LR
import tracks_pose_ref as T
from test_pose import rot_angle, seq as pose_seq, vec_angle  # noqa: F401 (fixture)
from test_scale import SCALE_ERR_ESTIMATED_POSE, seq as scale_seq  # noqa: F401 (fixture)


@pytest.fixture(scope="module")
def libs(pose_seq, scale_seq):
    return pose_seq, scale_seq


def test_rule1_slot_lists_on_hand_built_seen():
    L = 4
    seen = np.array([[0, 1, 2, 3, 4, 9, -3, 4],
                     [4, 4, 0, 0, 2, 1, 5, -1]])
    got = T.slot_lists(seen, L)
    want = [[2, 3, 4, 5, 7], [3, 4, 5, 7], [4, 5, 7],  # window 0: seen >= 2, >= 3, >= 4 (9 clamps to 4, -3 to 0)
            [0, 1, 4, 6], [0, 1, 6], [0, 1, 6]]
    assert len(got) == 2 * (L - 1)
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and g.tolist() == w
    # every list is a subset of its predecessor's inside a window
    for w in range(2):
        for k in range(1, L - 1):
            assert set(got[w * (L - 1) + k]) <= set(got[w * (L - 1) + k - 1])
    assert [len(x) for x in T.slot_lists(np.zeros((1, 5), int), 2)] == [0]
    assert T.slot_lists(np.full((1, 3), 1), 3)[0].tolist() == []  # seen once: in no pair


def test_join_on_the_slot_invariants(libs):
    for cs in T.gpu_cases():
        pairs = T.restate(libs, cs["K"], cs["tracks"], cs["seen"], **cs["kw"])
        assert len(pairs) == len(cs["patterns"]) * (cs["L"] - 1)
        for p in pairs:
            if p["k"] == 0:
                assert (p["scale"], p["triplets"], p["ratios"]) == (1.0, 0, 0), (cs["name"], p["w"])
            else:
                assert p["triplets"] == len(p["slots"]), (cs["name"], p["w"], p["k"])  # rule 4
                assert p["ratios"] <= max(p["triplets"] - 1, 0)
            assert len(p["pose"]["mask"]) == len(p["xyz"]) == len(p["valid"]) == len(p["slots"])
            assert 0.1 <= p["scale"] <= 5.0


def motion_errors(libs, seeds, **scene_kw):
    rot, tdir, scale = [], [], []
    for s in seeds:
        sc = LR.make_scene(s, W=4, slots=400, min_seen=4, **scene_kw)
        pairs = T.restate(libs, LR.K_KITTI, sc["tracks"][None], sc["seen"][None])
        truth = T.true_pairs(sc)
        for p, (R, t, length) in zip(pairs, truth):
            rot.append(rot_angle(p["pose"]["R"].T @ R))
            tdir.append(vec_angle(p["pose"]["t"], t))
            if p["k"] >= 1:
                want = length / truth[p["k"] - 1][2]
                scale.append(abs(p["scale"] - want) / want)
    return np.array(rot), np.array(tdir), np.array(scale)


SEEDS = range(12)
# Noiseless windows, poses ESTIMATED by the restatement (the scale tests' noiseless constant is for true poses, so it
# does not apply; the pixels are float32, so "noiseless" is a rounding of 6e-5 px): measured over seeds 0-11, three
# pairs each, bounded at 2 x the measured value
TRK_ROT_NOISELESS = 2 * 0.0046  # degrees; measured 0.00459
TRK_T_NOISELESS = 2 * 0.20  # degrees; measured 0.197
TRK_SCALE_NOISELESS = 2 * 9.4e-5  # relative; measured 9.37e-05


def test_known_motion_noiseless(libs):
    rot, tdir, scale = motion_errors(libs, SEEDS)
    print("noiseless: rot %.3g deg, t %.3g deg, scale %.3g" % (rot.max(), tdir.max(), scale.max()))
    assert rot.max() <= TRK_ROT_NOISELESS and tdir.max() <= TRK_T_NOISELESS and scale.max() <= TRK_SCALE_NOISELESS


# sigma = 0.3 px and 30 % outliers per frame >= 2: the class of test_sequential_pose_on_synthetic_scenes (rotation
# within 0.3 degrees) and of test_scale_with_estimated_poses_and_outliers (2 x SCALE_ERR_ESTIMATED_POSE).  The
# translation direction of these windows (depth 6-40 against the pose tests' 2-15, steps of 0.5-1.5) is a class of
# its own: measured over seeds 0-11
TRK_T_NOISY = 2 * 3.4  # degrees; measured 3.34


def test_known_motion_with_noise_and_outliers(libs):
    rot, tdir, scale = motion_errors(libs, SEEDS, sigma=0.3, outliers=0.3)
    print("noisy: rot %.3g deg, t %.3g deg, scale %.3g" % (rot.max(), tdir.max(), scale.max()))
    assert rot.max() <= 0.3
    assert tdir.max() <= TRK_T_NOISY
    assert scale.max() <= 2 * SCALE_ERR_ESTIMATED_POSE


def test_the_gpu_inputs_contain_the_classes_they_claim(libs):
    """tests/test_tracks_pose.py compares the GPU with this restatement on T.gpu_cases(): lists crossing 64 and 256
    positions, pairs of 0, 4 and 5 correspondences, a pair with triplets and no ratio, an all-dead window, and pairs
    that are really posed and scaled."""
    got = {}
    caps, lens, wins, iters = set(), set(), set(), set()
    for cs in T.gpu_cases():
        caps.add(cs["cap"]), lens.add(cs["L"]), wins.add(len(cs["patterns"])), iters.add(cs["kw"]["max_iters"])
        for k, v in T.classes(T.restate(libs, cs["K"], cs["tracks"], cs["seen"], **cs["kw"])).items():
            got[k] = got.get(k, False) or v
        seen = cs["seen"]
        got["seen_above_L"] = got.get("seen_above_L", False) or bool((seen > cs["L"]).any())
        got["seen_negative"] = got.get("seen_negative", False) or bool((seen < 0).any())
    assert all(got.values()), got
    assert caps == {1, 5, 63, 64, 65, 257, 300} and lens == {2, 3, 5} and iters == {0, 33, 1000}
    assert min(wins) == 1 and max(wins) == 7
