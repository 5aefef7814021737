"""Seeded random-input parity of the side paths on the GPU: N draws of tests/side_random.py per family, all on ONE
small context (sizes grow and shrink under the kernels from call to call), every fetched array against the expected
one bit for bit, floats as bit patterns.  tests/test_side_random_ref.py checks on the CPU that these very draws hold
the classes they are meant to and that the references agree with numpy.

N per family: the largest multiple of 8, not below 32, whose CPU side (generation, the sequential restatement and the
numpy reference of the CPU test) stays within 5 s on the build machine (measured with the machine idle; the times
vary by half as much again from run to run, so N sits a step below the edge).  A test that took more than 10 s on the
GPU has its N halved.

  family     N    CPU side   MI355X wall time (this module alone; generation included)
  matcher    144  4.3 s      1.5 s
  pose       640  4.5 s      1.0 s
  scale      320  4.7 s      0.7 s
  ba         48   4.7 s      3.3 s
  corners    32   0.7 s      11.6 s  (halved twice, to the floor: 12.8 s at 128, 12.4 s at 64.  About 11 s of it does
                                      not go with N -- the draws run at 10 ms each in the campaigns -- and shows only
                                      when this module runs alone and in this order: with 64 draws the test took 4.2 s
                                      as the first test of a run and under 2.3 s inside the whole suite.  It is the
                                      first family here that hands torch tensors to the library; where the constant
                                      comes from beyond that is not established.)
  tracks     640  4.4 s      2.6 s
  landmarks  96   4.0 s      1.7 s
  pnp        64   3.2 s      1.1 s   (halved from 128, 4.6 s on the CPU, which took 14.7 s as the first GPU test of a
                                      process -- it then pays what the corners test pays above, and compiles the three
                                      restatements it needs; 128 was not timed in this module's order)
  carry      128  4.1 s      1.3 s   (160 took 5.1 s on the CPU)
  reloc      96   3.7 s      1.6 s   (on its own five contexts, side_random.RELOC_CONTEXTS, one open at a time and
                                      the last one closed when the sweep ends: side_random.context)
"""
import pytest

import side_random as S

SEED = 20261020
N = dict(matcher=144, pose=640, scale=320, ba=48, corners=32, tracks=640, landmarks=96, pnp=64, carry=128, reloc=96)


def sweep(pkg, family):
    with S.context(pkg, family) as c:  # (reloc: its own contexts, closed when the block ends)
        for index in range(N[family]):
            d = S.draw(family, SEED, index)
            S.compare(family, S.run(family, c, d), d)  # (the message carries (family, seed, index))


@pytest.mark.gpu
def test_gpu_matcher_random(pkg):
    sweep(pkg, "matcher")


@pytest.mark.gpu
def test_gpu_pose_random(pkg):
    sweep(pkg, "pose")


@pytest.mark.gpu
def test_gpu_scale_random(pkg):
    sweep(pkg, "scale")


@pytest.mark.gpu
def test_gpu_ba_random(pkg):
    sweep(pkg, "ba")


@pytest.mark.gpu
def test_gpu_corners_random(pkg):
    sweep(pkg, "corners")


@pytest.mark.gpu
def test_gpu_tracks_chain_stitch_random(pkg):
    sweep(pkg, "tracks")


@pytest.mark.gpu
def test_gpu_landmarks_solve_write_back_random(pkg):
    sweep(pkg, "landmarks")


@pytest.mark.gpu
def test_gpu_window_pnp_random(pkg):
    sweep(pkg, "pnp")


@pytest.mark.gpu
def test_gpu_carry_and_carried_pnp_random(pkg):
    sweep(pkg, "carry")


@pytest.mark.gpu
def test_gpu_describe_points_and_reassociate_random(pkg):
    sweep(pkg, "reloc")  # (on side_random.RELOC_CONTEXTS, one after another: side_random.context)
