"""The window-pose chain and the write-back gate against an independent numpy restatement (CPU).

orbx_chain_window_poses (the library's host entry) and tests/cpp/wp_sequential.cpp (the sequential restatement, compiled
here with -ffp-contract=off) both compile csrc/orbx_wp_math.h; they have to agree bit for bit, and the 4x4 poses have
to be orbx_chain_trajectory's bit for bit.  tests/window_poses_ref.py restates the rules in numpy without sharing any
code.  Tolerance: that restatement evaluated in float64 and in numpy.longdouble on the inputs below, 16 x the largest
difference between the two (window_poses_ref.TOLERANCE records the value; the first test measures it again).

Inputs (window_poses_ref.cases): T0 identity, a rotation of exactly pi about a tilted axis (the quaternion branch) and
one of 1e-9 rad; windows of 2, 5 and 8 frames; a scale0 of 0.1 and one of 5; a degenerate pair (R = I, t = 0)."""
import math

import numpy as np
import pytest

import landmarks_ref as LR
import landmarks_seq as LS
import window_poses_ref as WR
import window_poses_seq as WS


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return WS.compile_seq(tmp_path_factory.mktemp("wp_seq_ref"))


@pytest.fixture(scope="module")
def reference():
    """the numpy restatement of every case, once: name -> (poses4x4, poses6, status)"""
    return {name: WR.chain(T0, R, t, s) for name, T0, R, t, s in WR.cases()}


def block_difference(got6, ref6):
    """largest difference of two sets of blocks; a rotation of pi has two rotation vectors, w and -w"""
    worst = 0.0
    for g, r in zip(np.asarray(got6, np.longdouble), np.asarray(ref6, np.longdouble)):
        dw = np.abs(g[:3] - r[:3]).max()
        if np.sqrt(np.sum(r[:3] ** 2)) > math.pi - 1e-6:
            dw = min(dw, np.abs(g[:3] + r[:3]).max())
        worst = max(worst, float(dw), float(np.abs(g[3:] - r[3:]).max()))
    return worst


def test_the_recorded_tolerance_is_the_measured_one(reference):
    worst = 0.0
    for name, T0, R, t, s in WR.cases():
        p4, p6, st = reference[name]
        q4, q6, _ = WR.chain(T0, R, t, s, dtype=np.longdouble)
        assert st == WR.OK
        worst = max(worst, float(np.abs(p4 - q4).max()), block_difference(p6, q6))
    for solved, built, term in WR.gate_cases_plain():
        p4 = WR.gate(solved, built, term)[0]
        q4 = WR.gate(solved, built, term, dtype=np.longdouble)[0]
        worst = max(worst, float(np.abs(p4 - q4).max()))
    print("float64 against longdouble: %.3g; 16 x = %.3g; recorded %.3g" % (worst, 16 * worst, WR.TOLERANCE))
    assert 0 < 16 * worst <= WR.TOLERANCE <= 32 * worst


def test_the_inputs_are_what_they_claim():
    T = WR.first_poses()
    assert T["identity"] is None
    R = T["pi"][:3, :3]
    assert 1.0 + np.trace(R) == 0.0 and np.abs(R @ R.T - np.eye(3)).max() < 1e-15  # exactly pi: the quaternion branch
    assert abs(np.linalg.norm(LR.rotvec(T["tiny"][:3, :3])) - 1e-9) < 1e-20
    names = [c[0] for c in WR.cases()]
    assert len(names) == len(set(names)) == 18
    assert {len(c[2]) + 1 for c in WR.cases()} == {2, 5, 8} and {c[4][0] for c in WR.cases()} == {0.1, 5.0}
    assert any((c[2][2] == np.eye(3)).all() and (c[3][2] == 0).all() for c in WR.cases() if len(c[2]) >= 3)


def test_host_entry_equals_numpy_within_the_tolerance(pkg, reference):
    for name, T0, R, t, s in WR.cases():
        p4, p6 = pkg.orbx_vo.chain_window_poses(T0, R, t, s)
        r4, r6, _ = reference[name]
        d4, d6 = float(np.abs(p4 - r4).max()), block_difference(p6, r6)
        print("%-18s 4x4 %.3g  blocks %.3g" % (name, d4, d6))
        assert d4 <= WR.TOLERANCE and d6 <= WR.TOLERANCE, name
    # the rotation of pi came through the branch 1 + tr R < 1e-3
    p6 = pkg.orbx_vo.chain_window_poses(WR.first_poses()["pi"], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0))[1]
    assert abs(np.linalg.norm(p6[0, :3]) - math.pi) < 1e-15


def test_host_entry_equals_the_sequential_restatement_bit_for_bit(pkg, seq):
    for name, T0, R, t, s in WR.cases():
        p4, p6 = pkg.orbx_vo.chain_window_poses(T0, R, t, s)
        ref = WS.seq_chain(seq, None if T0 is None else T0[None], s[:1], R[None], t[None], s[None])
        assert WS.bits_equal(p4, ref["poses4x4"][0]) and WS.bits_equal(p6, ref["poses6"][0]), name
        assert ref["status"][0] == WR.OK


def test_poses_are_chain_trajectory_bit_for_bit(pkg):
    for name, T0, R, t, s in WR.cases():
        p4, _ = pkg.orbx_vo.chain_window_poses(T0, R, t, s)
        assert WS.bits_equal(p4, pkg.chain_trajectory(np.eye(4) if T0 is None else T0, R, t, s)), name


def test_a_window_that_is_not_finite_says_so(pkg, seq):
    """a NaN or an infinity in any pair, in T0 or in scale0: NONFINITE for that window and for no other"""
    _, T0, R, t, s = WR.cases()[8]  # a window of 5 frames
    n = 5
    Rb, tb, sb = np.stack([R] * n), np.stack([t] * n), np.stack([s] * n)
    T0b, s0 = np.stack([np.eye(4) if T0 is None else T0] * n), sb[:, 0].copy()
    Rb[1, 2, 1, 1] = np.nan
    tb[2, 3, 0] = np.inf
    sb[3, 1] = np.nan
    s0[4] = np.inf
    ref = WS.seq_chain(seq, T0b, s0, Rb, tb, sb)
    assert ref["status"].tolist() == [WR.OK] + [WR.NONFINITE] * 4
    assert np.isfinite(ref["poses6"][0]).all() and not np.isfinite(ref["poses4x4"][1:]).all(axis=(1, 2, 3)).any()
    assert WR.chain(T0b[1], Rb[1], tb[1], sb[1])[2] == WR.NONFINITE


def test_gate_equals_numpy(seq):
    for solved, built, term in WR.gate_cases_plain():
        p4, upd, angle, dist = WS.seq_gate(seq, solved[None], built[None], [term], WR.MAX_ROT_DIFF, WR.MAX_TRANS_DIFF)
        r4, rupd, rangle, rdist = WR.gate(solved, built, term)
        assert np.abs(p4[0] - r4).max() <= WR.TOLERANCE
        assert np.abs(angle[0] - rangle).max() <= WR.TOLERANCE and np.abs(dist[0] - rdist).max() <= WR.TOLERANCE
        assert upd[0].tolist() == rupd.tolist()
        want = [1, 1, 0, 0] if term == WR.CONVERGENCE else [0, 0, 0, 0]  # 0.7 rad and 60 units are over the thresholds
        assert upd[0].tolist() == want, term
        # a pose that is not updated comes back as the inverse of its OLD block
        old4 = WR.gate(built, built, WR.SKIPPED)[0]
        for i in range(4):
            if not upd[0, i]:
                assert np.abs(p4[0, i] - old4[i]).max() <= WR.TOLERANCE


@pytest.fixture(scope="module")
def gate_reference(tmp_path_factory):
    """the gate scenes of the GPU test through the sequential build, solve and gate on the CPU"""
    tmp = tmp_path_factory.mktemp("wp_gate_ref")
    libs = (LS.compile_so(tmp, "lm_sequential"), LS.compile_so(tmp, "ba_sequential"), WS.compile_seq(tmp))
    return libs[2], WS.solve_scenes(libs[0], libs[1], LR.K_KITTI, *WR.gate_scenes())


def test_the_gate_scenes_fall_on_both_sides(gate_reference):
    """what tests/test_window_poses.py uploads really contains an updated and a refused pose for each threshold, a
    window that does not converge in one iteration and a skipped one"""
    seq, (built, solved, term, status) = gate_reference
    assert term[200].tolist() == [WR.CONVERGENCE] * 4 + [WR.SKIPPED] and status.tolist() == [LR.OK] * 4 + [LR.BASELINE]
    assert term[1].tolist() == [WR.NO_CONVERGENCE] * 4 + [WR.SKIPPED]
    _, upd, angle, dist = WS.seq_gate(seq, solved[200], built, term[200], WR.MAX_ROT_DIFF, WR.MAX_TRANS_DIFF)
    free = np.zeros(upd.shape, bool)
    free[:4, 1:] = True  # converged windows, the poses the solve may move
    # the standard rotation threshold is straddled: window 2 starts 0.7 rad off and converges
    assert (angle[free] > WR.MAX_ROT_DIFF).any() and (angle[free] < WR.MAX_ROT_DIFF).any()
    assert upd[2].tolist() == [1, 1, 0, 0] and upd[:2].all() and not upd[4].any()
    # the standard translation threshold is not (no scene converges from 50 units off): midpoints of the scenes' own
    assert dist.max() < WR.MAX_TRANS_DIFF
    max_rot, max_trans = WR.mid_thresholds(angle, dist, free)
    _, upd2, _, _ = WS.seq_gate(seq, solved[200], built, term[200], 10.0, max_trans)
    assert upd2[free].any() and not upd2[free].all()
    _, upd3, _, _ = WS.seq_gate(seq, solved[200], built, term[200], max_rot, 1e6)
    assert upd3[free].any() and not upd3[free].all()
    # no convergence: nothing is updated, whatever moved
    _, upd1, angle1, _ = WS.seq_gate(seq, solved[1], built, term[1], 10.0, 1e6)
    assert not upd1.any()
