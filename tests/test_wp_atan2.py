"""The atan2 restated in csrc/orbx_wp_math.h against glibc's, over the domain the log map reaches (CPU; DESIGN.md §9
rank 14).

wp_rodrigues_inv calls wp_atan2(s, q0) with the vector part's length s >= 0 and the scalar part q0 of a unit
quaternion: y >= 0, x of either sign, both in [0, 1] in magnitude.  The sweep below covers that domain -- 400 001
evenly spaced and 400 000 random angles in [0, pi] on the unit circle, 100 000 angles within 1e-18 .. 1 of each end,
and 200 000 of them scaled down by up to 1e-12 -- plus the values a sweep cannot hit: y = 0 with x = 1, -1, 0 and -0
(theta exactly 0 and exactly pi), x = 0 and -0 with y > 0 (pi / 2), and the smallest y beside x = -1 and x = 1.

Measured on this sweep: the largest difference from glibc's atan2 is 1 ulp (about a tenth of the arguments differ by
that one ulp; every special value is equal).  The assertion is that measured bound plus one ulp of margin."""
import ctypes as C

import numpy as np
import pytest

import landmarks_seq as LS

MEASURED_ULP = 1.0
BOUND_ULP = MEASURED_ULP + 1.0
SPECIAL = [  # (y, x, the value both must return)
    (0.0, 1.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.0), (0.0, -1.0, np.pi), (0.0, -0.0, np.pi), (0.0, -0.25, np.pi),
    (1.0, 0.0, np.pi / 2), (1.0, -0.0, np.pi / 2), (1e-300, -1.0, np.pi), (1e-300, 1.0, 1e-300),
    (5e-324, 1.0, 5e-324), (1.0, 1.0, np.pi / 4), (1.0, -1.0, 3 * np.pi / 4),
]


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return LS.compile_so(tmp_path_factory.mktemp("wp_seq"), "wp_sequential")


def wp_atan2(lib, y, x):
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(y)
    lib.seq_wp_atan2_many.restype = None
    lib.seq_wp_atan2_many(C.c_int(len(y)), y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                          out.ctypes.data_as(C.c_void_p))
    return out


def sweep():
    rng = np.random.default_rng(0)
    th = np.r_[np.linspace(0.0, np.pi, 400001), rng.uniform(0.0, np.pi, 400000), 10.0 ** rng.uniform(-18, 0, 100000),
               np.pi - 10.0 ** rng.uniform(-18, 0, 100000)]
    m = np.r_[np.ones(800001), 10.0 ** rng.uniform(-12, 0, 200000)]
    return np.abs(np.sin(th)) * m, np.cos(th) * m


def test_the_sweep_is_within_the_measured_bound(seq):
    y, x = sweep()
    assert (y >= 0).all() and (x < 0).any() and (x > 0).any() and max(y.max(), np.abs(x).max()) <= 1.0
    got, ref = wp_atan2(seq, y, x), np.arctan2(y, x)
    ulp = np.abs(got - ref) / np.spacing(np.maximum(np.abs(ref), 5e-324))
    print("largest difference from glibc: %g ulp, %.3f of the arguments differ" % (ulp.max(), (ulp > 0).mean()))
    assert ((got >= 0) & (got <= np.pi)).all()
    assert ulp.max() <= BOUND_ULP


def test_the_values_the_sweep_does_not_hit(seq):
    y, x, want = (np.array(c) for c in zip(*SPECIAL))
    got, ref = wp_atan2(seq, y, x), np.arctan2(y, x)
    assert got.tobytes() == ref.tobytes() == want.tobytes()


def test_a_nan_comes_back_as_a_nan(seq):
    got = wp_atan2(seq, [np.nan, 1.0, np.nan], [1.0, np.nan, np.nan])
    assert np.isnan(got).all()
