"""The draws tests/test_side_random.py runs on the GPU, checked on the CPU alone: for its fixed seeds, every family's
draws contain the classes its generator is there for (every boundary size, every parameter value, every kind of
result), and the sequential restatement that supplies the expected results agrees with its independent numpy
reference on the same draws -- within the tolerance the reference's own module records, no new one.

A decision the numpy reference flags as marginal (pose_ref.SAMPSON_FLAG, DEPTH_FLAG) excludes its draw from the
comparison; the excluded decisions may not exceed 1 in 500 of the compared ones per family (MARGINAL_CAP).

One line per family is printed: the classes found and the worst difference."""
import math

import numpy as np

import gftt_topup_ref as T
import landmarks_ref as LR
import landmarks_seq as LS
import landmarks_views_seq as VS
import oracle_lib as O
import pose_ref as P
import side_random as S
import stitch_ref as SR
import tracks_pose_ref as TR
import window_poses_ref as WR
import test_ba as BA
import test_matcher as M
import test_pose as TP
import test_pose_ref as TPR
import test_scale as TS
from test_side_random import N, SEED

MARGINAL_CAP = 1.0 / 500

_draws = {}


def draws(family):
    if family not in _draws:
        _draws[family] = [S.draw(family, SEED, i) for i in range(N[family])]
    return _draws[family]


def test_draws_depend_on_family_seed_and_index_only():
    for family in S.FAMILIES:
        a, b = S.draw(family, SEED, 5), S.draw(family, SEED, 5)
        S.compare(family, a["expected"], b)  # the expected result is reproducible
        other = S.draw(family, SEED + 1, 5)
        assert S.describe(family, a) == S.describe(family, b) != S.describe(family, other), family


def test_matcher_classes_and_numpy_against_the_oracle():
    ds = draws("matcher")
    assert {len(d["q"]) for d in ds} >= set(S.MATCH_SIZES) == {0, 1, 2, 63, 64, 65, 255, 256, 257, 513}
    assert {len(d["t"]) for d in ds} >= set(S.MATCH_SIZES)
    assert {d["ratio"] for d in ds} == {0.7, 0.8, 1.0}
    assert {d["kind"] for d in ds} == {"near", "tie_heavy", "duplicates", "identical"}
    both = [(len(d["q"]), len(d["t"])) for d in ds if len(d["q"]) in S.MATCH_SIZES and len(d["t"]) in S.MATCH_SIZES]
    assert len(both) >= N["matcher"] // 10  # query and train count on a boundary at once
    ties1 = ties2 = exact = kept = no_second = queries = 0
    for d in ds:
        idx, dist = d["expected"]["idx"], d["expected"]["dist"]
        oi, od = O.knn2(d["q"], d["t"])  # the C oracle: the restatement the hand-picked GPU tests compare with
        assert np.array_equal(oi, idx) and np.array_equal(od, dist), (d["seed"], d["index"])
        for a, b in zip(O.match_ratio(d["q"], d["t"], d["ratio"]), d["expected"]["match"]):
            assert np.array_equal(a, b), (d["seed"], d["index"])
        two = idx[:, 1] >= 0
        ties1 += int((two & (dist[:, 0] == dist[:, 1])).sum())
        if len(d["t"]) >= 3 and len(d["q"]):  # the second and the third neighbour tie: the lower index is kept
            qb, tb = (np.unpackbits(a, axis=1).astype(np.int32) for a in (d["q"], d["t"]))
            full = np.sort(qb @ (1 - tb).T + (1 - qb) @ tb.T, axis=1)
            ties2 += int((full[:, 1] == full[:, 2]).sum())
        exact += int((dist[:, 0] == 0).sum())
        kept += len(d["expected"]["match"][0])
        no_second += int((~two).sum())
        queries += len(idx)
    assert min(ties1, ties2, exact, kept, no_second) > 0
    print("matcher: %d draws, %d queries, %d matches kept, %d exact copies, %d ties on the first / %d on the second "
          "neighbour, %d queries without a second neighbour; numpy == oracle on all" %
          (len(ds), queries, kept, exact, ties1, ties2, no_second))


def test_pose_classes_and_restatement_against_numpy():
    ds = draws("pose")
    seq = S.seq_lib("pose")
    assert {len(d["p1"]) for d in ds} >= set(S.POSE_N) == {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129}
    assert max(len(d["p1"]) for d in ds) > 200
    assert {d["kw"]["max_iters"] for d in ds} >= set(S.POSE_ITERS) == {0, 1, 31, 32, 33, 64, 65}
    assert {d["kw"]["prob"] for d in ds} == {0.5, 0.99, 0.999}
    assert {d["kw"]["threshold"] for d in ds} == {0.5, 1.0, 2.0}
    assert {d["K"][0, 0] for d in ds} == {TP.K_KITTI[0, 0], TP.K_ANISO[0, 0]}
    assert any(d["kw"]["seed"] < 2**32 for d in ds) and any(d["kw"]["seed"] >= 2**32 for d in ds)
    assert {d["variant"] for d in ds} == {"plain", "repeated", "equal"}
    assert min(d["outliers"] for d in ds) < 0.1 and max(d["outliers"] for d in ds) > 0.5
    kinds = set()
    for d in ds:
        r, n, mi = d["expected"], len(d["p1"]), d["kw"]["max_iters"]
        if n < 5:
            assert TP.zero_result(r, n) and r["iters"] == 0
            kinds.add("n < 5")
        elif r["inliers"] == 0:
            assert TP.zero_result(r, n) and r["iters"] == mi
            kinds.add("no model")
        else:
            kinds.add("model")
            assert r["good"] == r["mask"].sum() <= r["inliers"]
            # where the run ended: by the stopping rule inside the first chunk of 32, on the chunk's edge, beyond it,
            # or at max_iters
            if r["iters"] < mi:
                kinds.add("stopped in the first chunk" if r["iters"] < 32 else
                          "stopped on the chunk edge" if r["iters"] == 32 else "stopped in a later chunk")
            else:
                kinds.add("ran to max_iters below 32" if mi < 32 else "ran to max_iters of 32" if mi == 32 else
                          "ran to max_iters beyond 32")
    want = {"n < 5", "no model", "model", "stopped in the first chunk", "stopped in a later chunk",
            "ran to max_iters below 32", "ran to max_iters of 32", "ran to max_iters beyond 32"}
    assert kinds >= want, want - kinds
    # the restatement against numpy (tests/pose_ref.py), as tests/test_pose_ref.py compares them
    decisions = excluded = tied = 0
    worst = 0.0
    for d in ds:
        got, kw, what = d["expected"], d["kw"], (d["seed"], d["index"])
        ref = P.ref_pose(d["p1"], d["p2"], d["K"], kw["prob"], kw["threshold"], kw["max_iters"], kw["seed"],
                         lambda *a: TPR.solve5_seq(seq, *a))
        n = len(d["p1"])
        if ref["flag_sampson"] or ref["flag_depth"]:
            excluded += n
            continue
        decisions += n
        assert (got["iters"], got["inliers"]) == (ref["iters"], ref["inliers"]), what
        assert np.array_equal(got["E"], ref["E"]), what
        if ref["inliers"] == 0:
            continue
        top = max(ref["cand_good"])
        first = [c for c in ref["candidates"] if c[2] == top]
        tied += len(first) > 1
        assert any(TPR.same_candidate(got, c) for c in first), what
        c = [c for c in first if TPR.same_candidate(got, c)][0]
        worst = max(worst, np.abs(got["R"] - c[0]).max(), np.abs(got["t"] - c[1]).max())
    print("pose: %d draws, kinds %s; %d decisions compared, %d excluded as marginal, %d tied candidates, worst R / t "
          "difference %.3g (bound %.3g)" % (len(ds), sorted(kinds), decisions, excluded, tied, worst, TPR.RUN_RT_BOUND))
    assert excluded <= MARGINAL_CAP * decisions, (excluded, decisions)


def test_scale_classes_and_restatement_against_numpy():
    ds = draws("scale")
    seq = S.seq_lib("scale")
    for k in (0, 1):  # the lengths of the scale call's lists
        assert {len(d["lists"][k]) for d in ds} >= set(S.SCALE_N) == {0, 1, 2, 255, 256, 257}
    assert {len(d["tri"][0][0]) for d in ds} >= set(S.SCALE_N)
    assert {d["pose"] for d in ds} == {"true", "degenerate"}
    assert {d["kind"] for d in ds} == {"triangulated", "noisy", "lattice", "far"}
    flags = set()
    w0 = invalid = points = 0
    classes = set()
    worst = 0.0
    for d in ds:
        prev, cur, pv, cv = d["lists"]
        for side, v in (("prev", pv), ("cur", cv)):
            flags.add((side, "NULL" if v is None else "all-zero" if not v.any() else "some"))
        if len(prev) != len(cur):
            classes.add("unequal lengths")
        # rule 3 in float32 numpy: bit for bit
        ref = TS.np_scale(prev, cur, pv, cv)
        assert d["expected"]["scale"] == ref, (d["seed"], d["index"], d["expected"]["scale"], ref)
        s, used = ref
        classes.add("no ratio" if used == 0 else "clamped at 0.1" if s == 0.1 else "clamped at 5" if s == 5.0 else
                    "even count" if used % 2 == 0 else "odd count")
        ratios, dropped = plain_ratios(prev, cur, pv, cv)
        if dropped:
            classes.add("overflowing distance")
        if len(ratios) >= 2 and ratios[len(ratios) // 2] == ratios[len(ratios) // 2 - 1]:
            classes.add("equal ratios at the median")
        # rules 1 and 2: numpy's SVD on the sound correspondences, the validity rule on all
        for k, ((p, q, R, t), (xyz, valid)) in enumerate(zip(d["tri"], d["expected"]["tri"])):
            h = TS.seq_homogeneous(seq, p, q, R, t)
            w0 += int((h[:, 3] == 0).sum())
            invalid += int((valid == 0).sum())
            points += len(p)
            assert not xyz[valid == 0].any()
            reg = d["regular"][k]
            if reg.any():
                assert valid[reg].all()
                got = h[reg, :3] / h[reg, 3:]
                ref3 = TS.svd_points(p[reg], q[reg], R, t)
                rel = np.linalg.norm(got - ref3, axis=1) / np.linalg.norm(ref3, axis=1)
                worst = max(worst, rel.max())
    assert flags == {(s, k) for s in ("prev", "cur") for k in ("NULL", "all-zero", "some")}, flags
    want = {"unequal lengths", "no ratio", "clamped at 0.1", "clamped at 5", "even count", "odd count",
            "overflowing distance", "equal ratios at the median"}
    assert classes >= want, want - classes
    assert w0 > 0 and invalid >= w0
    print("scale: %d draws, %d points triangulated (%d with w = 0, %d invalid), classes %s; rule 3 == float32 numpy on "
          "all, triangulation vs numpy.linalg.svd worst relative difference %.3g (bound %.3g)" %
          (len(ds), points, w0, invalid, sorted(classes), worst, TS.TRI_SVD_BOUND))
    assert worst <= TS.TRI_SVD_BOUND


def plain_ratios(prev, cur, pv, cv):
    """the sorted finite ratios of rule 3 and the number dropped for not being finite (float32 numpy)"""
    m = min(len(prev), len(cur))
    pv = np.ones(len(prev), bool) if pv is None else np.asarray(pv, bool)
    cv = np.ones(len(cur), bool) if cv is None else np.asarray(cv, bool)
    out, dropped = [], 0
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(1, m):
            if pv[i] and pv[i - 1] and cv[i] and cv[i - 1]:
                dp, dc = prev[i] - prev[i - 1], cur[i] - cur[i - 1]
                a = np.sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2])
                b = np.sqrt((dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2])
                r = float(a) / (float(b) + 1e-6)
                if math.isfinite(r):
                    out.append(r)
                else:
                    dropped += 1
    return sorted(out), dropped


def test_ba_classes_and_reported_costs():
    ds = draws("ba")
    wins = [(w, e, d) for d in ds for w, e in zip(d["windows"], d["expected"])]
    win_names = [n for d in ds for n in d["names"]]
    assert {len(d["windows"]) for d in ds} >= {1, 12} and all(1 <= len(d["windows"]) <= 12 for d in ds)
    assert {len(w["poses0"]) for w, _, _ in wins} == {2, 3, 4, 5, 6, 7, 8}
    assert {len(w["pts0"]) for w, _, _ in wins} >= set(S.BA_LANDMARKS) == {1, 7, 63, 256, 257}
    assert {d["delta"] for d in ds} == {1.0, 2.5}
    assert min(d["max_iters"] for d in ds) <= 3 and max(d["max_iters"] for d in ds) >= 25
    assert all(1 <= d["max_iters"] <= 30 for d in ds)
    names = {n for d in ds for n in d["names"]}
    assert any(" s0 " in n for n in names) and any(" s0.3 " in n for n in names)
    assert any(n.endswith("o0.2") or n.endswith("o0.2 hard") for n in names) and any(" o0" in n for n in names)
    degenerate = {n for n, _, _, _ in BA.degenerate_windows()}
    assert len(names & degenerate) >= 3, names & degenerate
    terms = {e[2]["termination"] for _, e, _ in wins}
    assert terms == {BA.CONVERGENCE, BA.NO_CONVERGENCE, BA.FAILURE}
    count = {t: sum(e[2]["termination"] == t for _, e, _ in wins) for t in sorted(terms)}
    worst = 0.0
    rejected = costs = 0
    for (w, (poses, pts, s), d), name in zip(wins, win_names):
        rejected += s["successful_steps"] < s["iterations"]
        if s["termination"] != BA.CONVERGENCE:  # the blocks are the inputs, bit for bit
            assert np.array_equal(poses, w["poses0"]) and np.array_equal(pts, w["pts0"])
            continue
        # the reported cost is numpy's cost of the returned blocks, within the bound of
        # test_noisy_windows_against_dense_numpy_lm and in its regime: residuals far above their own rounding.  A
        # projection of 1e3 px carries about 2e-12 px of rounding, so two programs' costs agree to about
        # 4e-12 / (rms residual in px) relatively: nine digits need an rms residual of 4e-3 px or more.  Windows
        # that end below 0.05 px (noiseless ones, and noisy ones with too few landmarks to be overdetermined) are
        # left to the bit-for-bit comparison on the GPU.
        if s["final_cost"] < 0.5 * len(w["obs_point"]) * 0.05 ** 2:
            continue
        costs += 1
        cost = BA.np_system(d["K"], poses, pts, w["obs_point"], w["obs_pose"], w["obs_xy"], d["delta"])[2]
        rel = abs(cost - s["final_cost"]) / max(s["final_cost"], 1e-300)
        worst = max(worst, rel)
        assert abs(cost - s["final_cost"]) <= 1e-9 * s["final_cost"] + 1e-300, (d["seed"], d["index"])
        assert s["final_cost"] <= s["initial_cost"]
    assert rejected > 0 and costs >= 20
    print("ba: %d draws, %d windows, terminations %s, %d windows with a rejected step; reported cost vs numpy's cost of "
          "the returned blocks on %d windows: worst relative difference %.3g (bound 1e-9)" %
          (len(ds), len(wins), count, rejected, costs, worst))


def test_corners_classes():
    """The corner entries' references are numpy already (tests/gftt_ref.py, tests/gftt_topup_ref.py): the classes only."""
    ds = draws("corners")
    assert {d["frames"].shape[2] for d in ds} >= set(S.GF_WIDTHS) == {63, 64, 65, 127, 128, 129}
    assert min(min(d["frames"].shape[1:]) for d in ds) <= 12 and max(max(d["frames"].shape[1:]) for d in ds) >= 150
    assert {len(d["frames"]) for d in ds} == {1, 2, 3, 4, 5, 6}
    assert {d["strided"] for d in ds} == {False, True}
    assert {d["quality"] for d in ds} == set(S.GF_QUALITY) == {0.001, 0.01, 0.1, 0.5}
    assert {d["dist"] for d in ds if d["dist"] <= 1.0} == {0.0, 0.5, 1.0}
    assert sum(1.0 < d["dist"] <= 12.0 and d["dist"] != round(d["dist"]) for d in ds) >= len(ds) // 4
    assert {d["max_corners"] for d in ds} == set(S.GF_MAX_CORNERS) == {1, 5, 64, 65, 2000}
    assert {d["masked_max"] for d in ds} == {0, 1, 5, 64, 65, 2000}  # 0: no limit
    assert {d["seeds"].shape[1] for d in ds} >= set(S.GF_SEED_COUNTS) == {1, 255, 256, 257}
    assert {d["seen_min"] for d in ds} == {0, 1, 2, 3} and any(d["seen"] is None for d in ds)
    assert {d["mask_kind"] for d in ds} == {"random", "empty", "full"}
    seen = set()
    frames = corners = 0
    for d in ds:
        nf, h, w = d["frames"].shape
        counts, carried, points, origin = d["expected"]["top"]
        for f in range(nf):
            sd = d["seeds"][f]
            live = np.ones(len(sd), bool) if d["seen"] is None else d["seen"][f] >= d["seen_min"]
            usable = T.usable_seeds(sd, w, h, None if d["seen"] is None else d["seen"][f], d["seen_min"])
            with np.errstate(invalid="ignore"):
                for name, m in (("NaN seed", np.isnan(sd).any(1)), ("infinite seed", np.isinf(sd).any(1)),
                                ("seed outside", np.isfinite(sd).all(1) & ((sd < 0).any(1) | (sd[:, 0] > w - 1) | (sd[:, 1] > h - 1))),
                                ("seed on the last column", sd[:, 0] == w - 1), ("seed on the last row", sd[:, 1] == h - 1)):
                    if (m & live).any():
                        seen.add(name)
                        # rule A: on the last row or column is inside, the other kinds are dropped
                        kept = np.isin(np.flatnonzero(m & live), usable)
                        assert kept.all() if name.startswith("seed on") else not kept.any(), name
            if (~live).any():
                seen.add("slot below seen_min")
            if len(usable) > d["max_corners"]:
                seen.add("slot capacity below the usable seeds")
                assert carried[f] == counts[f] == d["max_corners"]
            elif counts[f] == d["max_corners"] and counts[f] > carried[f]:
                seen.add("cap reached by new corners")
            elif counts[f] > carried[f]:
                seen.add("new corners below the cap")
            info = d["info"]["top"][f]
            n = len(info["indices"])
            seen.add("no candidate" if n == 0 else "candidates within the LDS sort" if n <= S.GF_LDS_KEYS else
                     "candidates beyond the LDS sort")
            if n >= 2 and (info["values"][1:] == info["values"][:-1]).any():
                seen.add("equal responses")
            if info["blocked"].all():
                seen.add("every pixel blocked")
            assert not points[f, counts[f]:].any() and (origin[f, counts[f]:] == -1).all()
            plain = d["expected"]["plain"][f]
            seen.add("plain cap reached" if len(plain) == d["max_corners"] else "plain below the cap")
            frames += 1
            corners += len(plain) + int(counts[f])
        n = len(d["info"]["masked"]["indices"])
        if d["masked_max"] == 0 and n > S.GF_LDS_KEYS:
            seen.add("masked, no limit, beyond the LDS sort")
        if d["mask_kind"] == "empty":
            assert len(d["expected"]["masked"]) == 0
        corners += len(d["expected"]["masked"])
    want = {"NaN seed", "infinite seed", "seed outside", "seed on the last column", "seed on the last row",
            "slot below seen_min", "slot capacity below the usable seeds", "cap reached by new corners",
            "new corners below the cap", "no candidate", "candidates within the LDS sort",
            "candidates beyond the LDS sort", "equal responses", "plain cap reached", "plain below the cap"}
    assert seen >= want, want - seen
    print("corners: %d draws, %d frames, %d corners expected, classes %s" % (len(ds), frames, corners, sorted(seen)))


def test_tracks_classes_and_chain_and_stitch_against_numpy():
    from test_window_poses_ref import block_difference

    ds = draws("tracks")
    assert {d["cap"] for d in ds} >= set(S.TRACK_SLOTS) == {1, 5, 63, 64, 65, 255, 256, 257}
    assert {d["L"] for d in ds} == {2, 3, 4, 5, 6}
    assert {len(d["patterns"]) for d in ds} == {1, 2, 3, 4, 5, 6, 7}
    assert {p for d in ds for p in d["patterns"]} == set(TR.PATTERNS)
    assert {d["stride"] for d in ds} == {1, 2, 3, 4, 5} and all(1 <= d["stride"] <= d["L"] - 1 for d in ds)
    assert any(d["stride"] == d["L"] - 1 for d in ds) and any(d["stride"] <= d["L"] - 2 for d in ds)
    assert all(d["stride"] <= d["L"] - 2 for d in ds if d["align"]) and {d["align"] for d in ds} == {False, True}
    assert any(d["T_start"] is None for d in ds) and any(d["T_start"] is not None for d in ds)
    assert {d["kw"]["max_iters"] for d in ds} >= set(S.POSE_ITERS) and max(d["kw"]["max_iters"] for d in ds) <= 100
    assert {d["K"][0, 0] for d in ds} == {TP.K_KITTI[0, 0], TP.K_ANISO[0, 0]}
    found = {}
    for d in ds:
        for k, v in TR.classes(d["pairs"]).items():
            found[k] = found.get(k, False) or v
    assert all(found.values()), found
    # the status codes.  The chain of a tracks block is finite (every pose is a rotation and a unit or zero t, every
    # scale is clamped to [0.1, 5]), so WR.NONFINITE and the stitch's BROKEN cannot be drawn here: they keep the tests
    # of their own (tests/test_window_poses.py, tests/test_stitch.py).
    wp_status = {int(v) for d in ds for v in d["expected"]["wp"]["status"]}
    st_status = {int(v) for d in ds for v in d["expected"]["st"]["status"]}
    assert wp_status == {WR.OK} and WR.NONFINITE not in wp_status
    assert st_status == {SR.OK, SR.SCALE_UNALIGNED} and SR.BROKEN not in st_status
    assert any((d["expected"]["st"]["lambda"] != 1.0).any() for d in ds)
    # the sequential chain and stitch against numpy, with the tolerances of their modules
    worst_wp = worst_st = 0.0
    windows = frames = 0
    for d in ds:
        tp, wp, st = (d["expected"][k] for k in ("tp", "wp", "st"))
        n, L = len(d["patterns"]), d["L"]
        R, t = tp["R"].reshape(n, L - 1, 3, 3), tp["t"].reshape(n, L - 1, 3)
        scale = tp["scale"].reshape(n, L - 1).copy()
        scale[:, 0] = d["s0"]
        for w in range(n):
            r4, r6, status = WR.chain(None, R[w], t[w], scale[w])
            d4, d6 = float(np.abs(wp["poses4x4"][w] - r4).max()), block_difference(wp["poses6"][w], r6)
            worst_wp = max(worst_wp, d4, d6)
            assert status == wp["status"][w] and d4 <= WR.TOLERANCE and d6 <= WR.TOLERANCE, (d["seed"], d["index"], w)
        case = dict(poses=wp["poses4x4"], T_start=d["T_start"])
        ref = SR.stitch(wp["poses4x4"], d["stride"], d["T_start"], d["align"], np.longdouble)
        dist, tol = SR.distance(st, ref), SR.tolerance(case, ref)
        worst_st = max(worst_st, dist / tol)
        assert dist <= tol, (d["seed"], d["index"], dist, tol)
        assert np.array_equal(st["owner"], ref["owner"]) and np.array_equal(st["status"], ref["status"])
        windows += n
        frames += len(st["owner"])
    print("tracks: %d draws, %d windows, %d pairs, %d stream frames, classes %s, stitch status %s; chain vs numpy worst "
          "%.3g (tolerance %.3g), stitch vs numpy in longdouble worst %.3g of its tolerance; no marginal decision "
          "excluded" % (len(ds), windows, sum(len(d["pairs"]) for d in ds), frames, sorted(found), sorted(st_status),
                        worst_wp, WR.TOLERANCE, worst_st))


def test_landmarks_classes_and_builds_against_numpy():
    from test_landmarks_views_ref import SVD_REL_BOUND, compare

    ds = draws("landmarks")
    lib = S.seq_lib("lm_views")
    assert {d["slots"] for d in ds} >= set(S.LM_SLOTS) == {1, 63, 64, 65, 257}
    assert {d["W"] for d in ds} == {2, 3, 4, 5, 6, 7, 8}
    assert {len(d["kinds"]) for d in ds} == {1, 2, 3, 4, 5, 6}
    assert {(d["build"], d["gate"]) for d in ds if d["build"] in S.LM_BUILDS[2:]} == \
        {(b, g) for b in ("first_two", "widest", "all_views") for g in (0.0, 3.0)}
    assert {d["build"] for d in ds} == set(S.LM_BUILDS)
    assert {d["min_seen"] == 0 for d in ds} == {False, True} and all(d["min_seen"] in (0, d["W"]) for d in ds)
    assert {k for d in ds for k in d["kinds"]} == set(S.LM_SCENES)
    assert all(1 <= d["max_iters"] <= 20 for d in ds) and {d["delta"] for d in ds} == {1.0, 2.5}
    status = {int(v) for d in ds for v in d["expected"]["block"]["status"]}
    assert status == {LR.OK, LR.BASELINE, LR.EMPTY, LR.BAD_POSE}
    reasons = {int(v) for d in ds if "reason" in d["expected"] for v in np.unique(d["expected"]["reason"])}
    assert reasons == {VS.KEPT, VS.SHORT, VS.DEGENERATE, VS.BEHIND, VS.REPROJECTION, VS.NO_WINDOW}
    terms = {sm["termination"] for d in ds for sm in d["expected"]["summaries"]}
    assert terms == {BA.CONVERGENCE, BA.NO_CONVERGENCE, BA.FAILURE, S.BA_SKIPPED}
    # no summary holds a NaN (side_random._lm_scene: which NaN is no rule's business), yet pixels that are not finite
    # are drawn, with and without a gate
    assert all(math.isfinite(sm["initial_cost"]) and math.isfinite(sm["final_cost"])
               for d in ds for sm in d["expected"]["summaries"])
    bad = {(d["build"] in S.LM_BUILDS[2:] and d["gate"] > 0) for d in ds for sc in d["scenes"] if "bad_slot" in sc}
    assert bad == {False, True}
    upd = np.concatenate([d["expected"]["updated"].ravel() for d in ds])
    assert upd.any() and not upd.all()
    # a window that converged and yet keeps a pose: the gate's thresholds decide, not the termination alone
    gated = sum(int(((d["expected"]["updated"][w, 1:] == 0).any()))
                for d in ds for w, sm in enumerate(d["expected"]["summaries"]) if sm["termination"] == BA.CONVERGENCE)
    # the builds against numpy: reasons equal wherever the decision is not marginal, points within SVD_REL_BOUND
    worst, compared, marginal, decisions = 0.0, 0, 0, 0
    for d in ds:
        mode = max(S.LM_BUILDS.index(d["build"]) - 2, 0)
        gate = d["gate"] if d["build"] in S.LM_BUILDS[2:] else 0.0
        if d["build"] in ("plain", "chained"):  # the build of rank 10 is the first-two build without a gate, bit for bit
            views = VS.seq_views_build(lib, d["K"], d["poses"], d["tracks"], d["seen"], VS.FIRST_TWO, 0.0)[0]
            LS.assert_blocks_equal(d["expected"]["block"], views)
        for w, sc in enumerate(d["scenes"]):
            sc = dict(sc, poses=d["poses"][w])
            if "bad_slot" in sc:  # numpy's SVD does not take a pixel that is not finite: the other slots of the window
                sc["seen"] = sc["seen"].copy()
                sc["seen"][sc["bad_slot"]] = 0
            w_, n, m = compare(lib, sc, mode, gate)
            worst, compared, marginal, decisions = max(worst, w_), compared + n, marginal + m, decisions + d["slots"]
    print("landmarks: %d draws, %d windows, status %s, reasons %s, terminations %s, %d converged windows with a pose the "
          "gate kept; builds vs numpy SVD: worst relative point difference %.3g (bound %.3g) over %d points, %d of %d "
          "decisions marginal" % (len(ds), sum(len(d["kinds"]) for d in ds), sorted(status), sorted(reasons),
                                  sorted(terms), gated, worst, SVD_REL_BOUND, compared, marginal, decisions))
    assert marginal <= MARGINAL_CAP * decisions, (marginal, decisions)
    assert worst <= SVD_REL_BOUND, worst
