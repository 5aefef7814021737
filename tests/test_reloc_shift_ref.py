"""CPU-only, the references alone: two 320 x 160 crops of kitti_000000 offset by the integer shift (7, 3) are joined by
descriptor.  gftt_ref finds the corners of both crops, reassoc_ref.describe_points describes them
on the oracle under rules A-E, reassoc_ref.reassociate_window joins them with ratio 0.8 and unique = 1.  A match is
right when its two points differ by exactly the shift.  Measured here, on the CPU: 200 corners in either crop, 156 and
158 of them ORBX_PD_OK, 150 matches, all 150 right, none wrong.  tests/test_reloc.py demands the device's origin equal
to this reference's element for element."""
import functools

import numpy as np

import gftt_ref as G
import oracle_lib as O
import reassoc_ref as R

Y0, X0, H, W = 100, 300, 160, 320  # the crop of smoke()
SHIFT = (7, 3)                     # crop B starts 7 px to the right of and 3 px below crop A
MAX_CORNERS, QUALITY, MIN_DISTANCE = 200, 0.01, 7.0
RATIO, MAX_DISTANCE, UNIQUE = 0.8, 256, 1
BLUR_LEVELS = 2                    # the level-0 image of smoke()'s parameters
RIGHT_AT_LEAST = 150               # measured: 150 right, 0 wrong


def crops():
    img = O.load_kitti(0)
    a = img[Y0:Y0 + H, X0:X0 + W].copy()
    b = img[Y0 + SHIFT[1]:Y0 + SHIFT[1] + H, X0 + SHIFT[0]:X0 + SHIFT[0] + W].copy()
    return a, b


@functools.lru_cache(maxsize=None)
def reference():
    """dict of the crops, their corners (200-slot arrays, zeros past the count), counts, the two described sets and the
    re-association with crop B as the query and crop A as the train set"""
    a, b = crops()
    params = O.gpu_params(blur_levels=BLUR_LEVELS)
    out = dict(crops=(a, b), corners=[], counts=[], described=[])
    for img in (a, b):
        c = G.good_features_to_track(img, MAX_CORNERS, QUALITY, MIN_DISTANCE)
        slots = np.zeros((MAX_CORNERS, 2), np.float32)
        slots[:len(c)] = c
        out["corners"].append(slots)
        out["counts"].append(len(c))
        out["described"].append(R.describe_points(img, slots, params, count=len(c)))
    da, db = out["described"]
    out["origin"], out["dist"], out["count"] = R.reassociate_window(db["desc"], db["state"], da["desc"], da["state"],
                                                                    RATIO, MAX_DISTANCE, UNIQUE)
    return out


def test_the_reference_joins_the_shifted_crops():
    ref = reference()
    ca, cb = ref["corners"]
    assert ref["counts"] == [MAX_CORNERS, MAX_CORNERS]
    assert [d["n_ok"] for d in ref["described"]] == [156, 158]
    assert all(d["nskip"] == 0 and d["noob"] == 0 for d in ref["described"])
    matched = np.flatnonzero(ref["origin"] >= 0)
    right = sum(np.array_equal(ca[ref["origin"][q]] - cb[q], np.float32(SHIFT)) for q in matched)
    wrong = len(matched) - right
    print("matches %d, right %d, wrong %d, largest distance %d" % (len(matched), right, wrong, ref["dist"].max()))
    assert wrong == 0 and right >= RIGHT_AT_LEAST and ref["count"] == len(matched)
    # every match joins two OK slots, and no train slot is taken twice
    da, db = ref["described"]
    assert (db["state"][matched] == R.PD_OK).all() and (da["state"][ref["origin"][matched]] == R.PD_OK).all()
    assert len(set(ref["origin"][matched].tolist())) == len(matched)
