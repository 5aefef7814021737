"""The buffers of the work beside the batched path grow under their users' feet and nobody notices (GPU).

Good features, the top-up, the LK windows tracker, landmarks (build + solve) and the tracks pose each own a workspace
and a result block per context, grown on demand by SideWork::grow while earlier calls may still be running on another
stream.  Here every path is called small, large, small on ONE context -- 2 then 6 frames of 96 x 64, 16 then 300 slots
(300 crosses one 256-thread pass), windows of 2 then 4 frames, min_distance 0, 1 and 8 -- so that the large call
grows every buffer of the path and the second small one runs in buffers larger than it needs, with the calls moving
between two caller streams and the context's own.  Every result has to be bit-equal to the same call on a fresh
context.  That is a consistency condition; correctness against the references stays with the parity tests of each
path.

Three arrangements:
 * the paths chained as a stream would chain them (corners -> windows -> top-up / tracks pose / landmarks), each
   stage on another stream than its producer and reading the producer's block in place, results fetched per call;
 * each path alone on inputs that stay put, the calls issued back to back with NO host synchronisation in between, so
   that a buffer grows while the previous call on another stream may still be using it;
 * the one-window / one-frame host entries, which stage their inputs in buffers of their own.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

W, H = 96, 64
K = np.array([[100.0, 0.0, 48.0], [0.0, 100.0, 32.0], [0.0, 0.0, 1.0]])
SMALL = dict(n=2, cap=16, L=2)
LARGE = dict(n=6, cap=300, L=4)
ORDER = (SMALL, LARGE, SMALL)
MIN_DISTANCE = (0.0, 1.0, 8.0)  # of the first, second and third call
QUALITY = 0.01
PATHS = ("good_features", "topup", "lk_windows", "landmarks", "tracks_pose")


def windows(z):
    return z["n"] - z["L"] + 1


def poses_of(nw, L):
    """poses that make the frames' shift a plane at some depth (as test_landmarks.rolled)"""
    p = np.zeros((nw, L, 6))
    for k in range(L):
        p[:, k, 3:] = (0.5 * k, k / 6.0, 0.0)
    return p


def flat(x):
    """a result of any fetch as a list of (dtype, shape, bytes): equal lists are bit-equal results"""
    if isinstance(x, dict):
        return [(k, flat(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [flat(a) for a in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


# ---- one call of each path; every input explicit, nothing waits for the device ----
def run_good_features(c, t, z, md, s):
    c.good_features_batch(t[:z["n"]], z["cap"], QUALITY, md, stream=s)


def run_lk_windows(c, t, z, points, counts, s):
    c.lk_track_windows(t[:z["n"]], list(range(windows(z))), z["L"], points, counts, slot_capacity=z["cap"], stream=s)


def run_topup(c, t, z, tracks, seen, md, s):
    """seeds: the last position of every window's tracks, on the window's last frame"""
    L, cap = z["L"], z["cap"]
    c.good_features_topup(t[L - 1:L - 1 + windows(z)], tracks + 8 * (L - 1), seen, L, seed_capacity=cap,
                          seed_point_stride=2 * L, seed_frame_stride=2 * L * cap, max_corners=cap,
                          quality_level=QUALITY, min_distance=md, stream=s)


def run_tracks_pose(c, z, tracks, seen, s):
    c.tracks_pose(K, tracks, seen, windows(z), z["cap"], z["L"], max_iters=50, stream=s)


def run_landmarks(c, z, tracks, seen, s_build, s_solve):
    c.landmarks_build(K, tracks, seen, poses_of(windows(z), z["L"]), n_windows=windows(z), slot_capacity=z["cap"],
                      window_len=z["L"], stream=s_build)
    c.bundle_adjust_landmarks(max_iters=10, stream=s_solve)


FETCH = dict(
    good_features=lambda c: c.good_features_fetch(),
    topup=lambda c: c.good_features_topup_fetch(),
    lk_windows=lambda c: c.lk_windows_fetch(),
    landmarks=lambda c: (c.landmarks_fetch(), c.bundle_adjust_landmarks_fetch()),
    tracks_pose=lambda c: (c.tracks_pose_fetch(),
                           [c.tracks_pose_pair_fetch(p) for p in range(c.tracks_pose_view().n_pairs)]),
)


def chain(c, t, z, md, s):
    """corners -> windows -> top-up, tracks pose, landmarks: each stage reads its producer's block in place, on
    another stream; then every path's results (each fetch waits for its path)"""
    run_good_features(c, t, z, md, s[0])
    g = c.good_features_view()
    assert g.slot_capacity == z["cap"]
    run_lk_windows(c, t, z, g.corners_xy, g.counts, s[1])
    v = c.lk_windows_view()
    run_topup(c, t, z, v.tracks_xy, v.seen, md, s[2])
    run_tracks_pose(c, z, v.tracks_xy, v.seen, s[0])
    run_landmarks(c, z, v.tracks_xy, v.seen, s[2], s[1])
    return {p: FETCH[p](c) for p in PATHS}


def context(pkg):
    return pkg.Context(pkg.default_params("gpu", max_width=W, max_height=H, max_batch=LARGE["n"]))


@pytest.fixture(scope="module")
def frames():
    """6 frames: a 96 x 64 crop of kitti_000000 (road: more than 300 corners) rolled by (1, 3) pixels per frame"""
    crop = np.ascontiguousarray(O.load_kitti(0)[300:300 + H, 480:480 + W])
    return np.stack([np.roll(crop, (k, 3 * k), axis=(0, 1)) for k in range(LARGE["n"])])


@pytest.fixture(scope="module")
def streams(pkg):
    """two caller streams and the context's own (None)"""
    hip = pkg.orbx.load()
    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    yield (sa.value, sb.value, None)
    assert hip.hipStreamDestroy(sa) == 0 and hip.hipStreamDestroy(sb) == 0


@pytest.fixture(scope="module")
def device_frames(frames):
    import torch

    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def fresh(pkg, device_frames, streams):
    """call i of ORDER on a context of its own: what the other contexts have to reproduce"""
    out = []
    for z, md in zip(ORDER, MIN_DISTANCE):
        with context(pkg) as c:
            out.append(chain(c, device_frames, z, md, streams))
    return out


@pytest.fixture(scope="module")
def chained(pkg, device_frames, streams):
    """the three calls on one context, the streams moving on by one from call to call"""
    with context(pkg) as c:
        return [chain(c, device_frames, z, md, streams[i:] + streams[:i])
                for i, (z, md) in enumerate(zip(ORDER, MIN_DISTANCE))]


def test_the_shapes_exercise_the_paths(fresh):
    """not a comparison of nothing with nothing: corners found, most of them tracked, landmarks built and solved"""
    for r, z in zip(fresh, ORDER):
        nw = windows(z)
        assert len(r["good_features"]) == z["n"] and min(len(a) for a in r["good_features"]) >= min(z["cap"], 10)
        tracks, seen, err = r["lk_windows"]
        assert tracks.shape == (nw, z["cap"], z["L"], 2) and (seen == z["L"]).sum() >= 8 * nw
        counts, carried, points, origin = r["topup"]
        assert points.shape == (nw, z["cap"], 2) and carried.min() >= 8 and (counts >= carried).all()
        block, (poses, summaries, pts) = r["landmarks"]
        assert len(block["status"]) == nw and len(summaries) == nw and poses.shape == (nw, z["L"], 6)
        assert r["tracks_pose"][0]["n"].shape == (nw * (z["L"] - 1),) and r["tracks_pose"][0]["n"].max() >= 8
    assert len(fresh[1]["good_features"][0]) > 256  # more than one 256-thread pass


@pytest.mark.parametrize("path", PATHS)
def test_chained_calls_equal_a_fresh_context(chained, fresh, path):
    for i in range(len(ORDER)):
        assert flat(chained[i][path]) == flat(fresh[i][path]), (path, i)


@pytest.fixture(scope="module")
def inputs(fresh, device_frames):
    """what each path reads, per call of ORDER, uploaded once and left alone: the corners as the tracker's points, the
    tracks and seen counts as the seeds and as the input of landmarks and tracks pose"""
    import torch

    out = []
    for r, z in zip(fresh, ORDER):
        nw = windows(z)
        pts = np.zeros((nw, z["cap"], 2), np.float32)
        for w in range(nw):
            pts[w, :len(r["good_features"][w])] = r["good_features"][w]
        counts = np.int32([len(r["good_features"][w]) for w in range(nw)])
        tracks, seen, _ = r["lk_windows"]
        out.append({k: torch.from_numpy(a).cuda() for k, a in
                    dict(points=pts, counts=counts, tracks=tracks, seen=seen).items()})
    torch.cuda.synchronize()
    return out


def call(path, c, t, i, x, s):
    z, md = ORDER[i], MIN_DISTANCE[i]
    if path == "good_features":
        run_good_features(c, t, z, md, s[0])
    elif path == "topup":
        run_topup(c, t, z, x["tracks"].data_ptr(), x["seen"].data_ptr(), md, s[0])
    elif path == "lk_windows":
        run_lk_windows(c, t, z, x["points"].data_ptr(), x["counts"].data_ptr(), s[0])
    elif path == "landmarks":
        run_landmarks(c, z, x["tracks"].data_ptr(), x["seen"].data_ptr(), s[0], s[1])
    else:
        run_tracks_pose(c, z, x["tracks"].data_ptr(), x["seen"].data_ptr(), s[0])


@pytest.mark.parametrize("calls", [2, 3])
@pytest.mark.parametrize("path", PATHS)
def test_back_to_back_calls_equal_a_fresh_context(pkg, device_frames, streams, fresh, inputs, path, calls):
    """the first `calls` calls of ORDER without a host synchronisation in between, each on the next stream: the large
    call grows the buffers the small one may still be using; what the last call left is the fresh context's"""
    with context(pkg) as c:
        for i in range(calls):
            call(path, c, device_frames, i, inputs[i], streams[i:] + streams[:i])
        got = FETCH[path](c)
    assert flat(got) == flat(fresh[calls - 1][path])


def test_window_and_pose_tables_grow(pkg, device_frames, streams, fresh, inputs):
    """1, 70, 1 windows of 16 slots over the six frames: the window table outgrows its first 256 bytes and the pose
    table's pinned mirror its first 4096"""
    z = dict(n=6, cap=16, L=4)
    firsts = ([0], [k % 3 for k in range(70)], [0])
    x = inputs[0]

    def run(c, i):
        nw, s = len(firsts[i]), streams[i:] + streams[:i]
        pts, cnt = x["points"].expand(nw, -1, -1).contiguous(), x["counts"].expand(nw).contiguous()
        c.lk_track_windows(device_frames, firsts[i], z["L"], pts, cnt, stream=s[0])
        v = c.lk_windows_view()
        c.landmarks_build(K, v.tracks_xy, v.seen, poses_of(nw, z["L"]), n_windows=nw, slot_capacity=z["cap"],
                          window_len=z["L"], stream=s[1])
        c.bundle_adjust_landmarks(max_iters=10, stream=s[2])
        return flat((FETCH["lk_windows"](c), FETCH["landmarks"](c)))

    import torch

    torch.cuda.synchronize()
    with context(pkg) as c:
        got = [run(c, i) for i in range(3)]
    for i in range(3):
        with context(pkg) as c:
            assert run(c, i) == got[i], i
    assert got[0] == got[2]


def test_host_entries_equal_a_fresh_context(pkg, frames, fresh):
    """the one-frame and one-window host entries stage their inputs in buffers of their own (image, seeds or mask,
    frames and points, tracks | seen): a 48 x 32 corner of the frame, the whole frame, the corner again"""
    def run(c, i):
        z, md = ORDER[i], max(MIN_DISTANCE[i], 1.0)
        img = frames[0] if z is LARGE else np.ascontiguousarray(frames[0][:32, :48])
        mask = np.ones_like(img)
        mask[::3] = 0
        corners = c.good_features_to_track(img, z["cap"], 0.01, md)
        tracks, seen, _ = fresh[i]["lk_windows"]
        L = z["L"]
        seq = frames[:L] if z is LARGE else np.ascontiguousarray(frames[:L, :32, :48])
        return flat((corners, c.good_features_to_track_masked(img, mask, z["cap"], 0.01, md),
                     c.good_features_topup_one(img, corners[:8], z["cap"], 0.01, md),
                     c.lk_track_window(seq, corners),
                     c.bundle_adjust_tracks(K, tracks[0], seen[0], poses_of(1, L)[0], max_iters=10),
                     c.tracks_pose_window(K, tracks[0], seen[0], max_iters=50)))

    with context(pkg) as c:
        got = [run(c, i) for i in range(3)]
    for i in range(3):
        with context(pkg) as c:
            assert run(c, i) == got[i], i
