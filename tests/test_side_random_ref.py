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
import pnp_seq as PS
import pose_ref as P
import reassoc_ref as RR
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


def ransac_classes(records, max_iters, into):
    """where the runs of a records array ended: inside the first chunk of 64 by the stopping rule, on the chunk's
    edge, in a later chunk, or at max_iters"""
    for r in records.ravel():
        if r["status"] != PS.OK:
            continue
        it = int(r["iters"])
        into.add("ended on the edge of the first chunk" if it == S.PNP_CHUNK else
                 "ran to max_iters" if it == max_iters else
                 "stopped in the first chunk" if it < S.PNP_CHUNK else "stopped in a later chunk")


RANSAC_WANT = {"stopped in the first chunk", "ended on the edge of the first chunk", "stopped in a later chunk",
               "ran to max_iters"}


def assert_pnp_parameters(ds):
    ps = [d["params"] for d in ds]
    assert {p["max_iters"] for p in ps} == set(S.PNP_ITERS) == {0, 1, 63, 64, 65, 128, 300}
    assert {p["prob"] for p in ps} == set(S.PNP_PROB) == {0.5, 0.99, 0.999}
    assert {p["threshold_px"] for p in ps} == set(S.PNP_THRESHOLD) == {0.5, 1.0, 2.0}
    assert {p["refine_iters"] for p in ps} == set(S.PNP_REFINE) == {0, 1, 10, 20}
    assert {p["min_inliers"] for p in ps} == set(S.PNP_MIN_INLIERS) == {4, 30}
    assert any(p["seed"] < 2**32 for p in ps) and any(p["seed"] >= 2**32 for p in ps)


def size_classes(rec, cap, into):
    ok = rec["status"] == PS.OK
    for name, m in (("n_corr > 256", rec["n_corr"] > S.PNP_LANES), ("inliers > 256", ok & (rec["inliers"] > S.PNP_LANES)),
                    ("256 < n_corr < cap", (rec["n_corr"] > S.PNP_LANES) & (rec["n_corr"] < cap)),
                    ("n_corr == cap", rec["n_corr"] == cap)):
        if m.any():
            into.add(name)


SIZE_WANT = {"n_corr > 256", "inliers > 256", "256 < n_corr < cap", "n_corr == cap"}


def test_pnp_classes_and_restatement_against_the_true_poses():
    import pnp_ref as PR

    ds = draws("pnp")
    assert {d["cap"] for d in ds} >= set(S.PNP_SLOTS) == {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513}
    assert max(d["cap"] for d in ds) <= 600 and sum(d["cap"] not in S.PNP_SLOTS for d in ds) >= len(ds) // 4
    assert {d["W"] for d in ds} == set(S.PNP_WINDOW_LEN) == {3, 4, 5, 8}
    assert {len(d["kinds"]) for d in ds} == {1, 2, 3, 4, 5, 6}
    assert {k for d in ds for k in d["kinds"]} == set(S.PNP_KINDS)
    assert_pnp_parameters(ds)
    assert sum(d["host"] is not None for d in ds) == len(ds) // 2
    assert sum(d["solve"] is not None for d in ds) >= 2 and all(d["cap"] <= 257 for d in ds if d["solve"] is not None)
    status, stops, sizes = set(), set(), set()
    for d in ds:
        rec = d["expected"]["pnp"]["records"]
        status |= {int(v) for v in rec["status"].ravel()}
        ransac_classes(rec, d["params"]["max_iters"], stops)
        size_classes(rec, d["cap"], sizes)
        # a record that is not OK is empty but for its counts, and its pose is the built one
        bad = rec["status"] != PS.OK
        assert not rec["inliers"][bad].any() and not rec["rms_px"][bad].any() and not d["expected"]["pnp"]["mask"][bad].any()
        assert d["expected"]["pnp"]["poses6"][:, 2:][bad].tobytes() == d["poses"][:, 2:][bad].tobytes()
        assert d["expected"]["pnp"]["poses6"][:, :2].tobytes() == d["poses"][:, :2].tobytes()
    assert status == {PS.OK, PS.SKIPPED, PS.FEW_POINTS, PS.NO_MODEL}, status
    assert stops >= RANSAC_WANT, RANSAC_WANT - stops
    assert sizes >= SIZE_WANT, SIZE_WANT - sizes
    host_status = {d["expected"]["host"]["status"] for d in ds if d["host"] is not None}
    terms = {sm["termination"] for d in ds if d["solve"] is not None for sm in d["expected"]["solve"]["summaries"]}
    # the restatement's poses against the scene's true ones, within the bounds tests/test_pnp.py asserts on the device
    # (1e-4 rad, 1e-2 units; the poses were handed out 2e-3 off).  The windows are chosen by what they were drawn as,
    # not by how they came out: clean or padded, or at most 30 % outliers (those have no pixel noise) under a max_iters
    # of 63 or more (a sample of three is free of outliers with probability 0.34 or more: none in 63 has a chance below
    # 1e-11, while a max_iters of 1 leaves the one sample's model, OK with a dozen inliers), with at least 30 slots that
    # own a landmark; every OK problem of such a window is compared.
    worst_r = worst_t = 0.0
    compared = ok_windows = chosen = 0
    for d in ds:
        rec = d["expected"]["pnp"]["records"]
        for w, (kind, sc) in enumerate(zip(d["kinds"], d["scenes"])):
            has_ok = bool((rec["status"][w] == PS.OK).any())
            ok_windows += has_ok
            few = kind == "outliers" and d["shares"][w] <= 0.3 and d["params"]["max_iters"] >= 63
            if not (kind in ("clean", "padded") or few) or d["live"][w] < 30:
                continue
            chosen += has_ok
            for k in range(2, d["W"]):
                if rec["status"][w, k - 2] != PS.OK:
                    continue
                er, et = PR.pose_error(d["expected"]["pnp"]["poses6"][w, k], LR.rodrigues(sc["true_poses"][k, :3]),
                                       sc["true_poses"][k, 3:])
                worst_r, worst_t, compared = max(worst_r, er), max(worst_t, et), compared + 1
                assert er < 1e-4 and et < 1e-2, (d["seed"], d["index"], w, k, er, et)
    assert 3 * chosen >= ok_windows and compared >= 30, (chosen, ok_windows, compared)
    print("pnp: %d draws, %d windows, %d problems, status %s, host-entry status %s, seeded-solve terminations %s, "
          "classes %s; PnP pose vs the true pose on %d problems of %d of %d windows with an OK problem: worst %.3g rad "
          "(bound 1e-4), %.3g units (bound 1e-2)" % (
              len(ds), sum(len(d["kinds"]) for d in ds), sum(d["expected"]["pnp"]["records"].size for d in ds),
              sorted(status), sorted(host_status), sorted(terms), sorted(stops | sizes), compared, chosen, ok_windows,
              worst_r, worst_t))


def test_carry_classes_and_join_against_a_dictionary():
    ds = draws("carry")
    assert {d["cap"] for d in ds} >= set(S.CARRY_SLOTS) == {1, 5, 63, 64, 65, 255, 256, 257, 513}
    assert {d["old_cap"] for d in ds} >= set(S.CARRY_SLOTS)
    assert sum(d["cap"] in S.CARRY_SLOTS and d["old_cap"] in S.CARRY_SLOTS for d in ds) >= len(ds) // 10
    assert max(max(d["cap"], d["old_cap"]) for d in ds) <= 600 and any(d["cap"] != d["old_cap"] for d in ds)
    assert {d["W"] for d in ds} == set(S.PNP_WINDOW_LEN) == {3, 4, 5, 8}
    assert {len(d["kinds"]) for d in ds} == {1, 2, 3, 4, 5, 6}
    assert {k for d in ds for k in d["kinds"]} == set(S.CARRY_KINDS)
    assert {d["solve"] is None for d in ds} == {False, True}
    assert_pnp_parameters(ds)
    origins, status, wstatus, stops, sizes, old_status = set(), set(), set(), set(), set(), set()
    slots = carried = 0
    for d in ds:
        block, carry, loc = (d["expected"][k] for k in ("block", "carry", "loc"))
        src = block["points3"] if d["points"] is None else d["points"]
        old_status |= {int(v) for v in block["status"]}
        # rule A by a dictionary look-up of each window's slot_of_point
        for w in range(len(d["kinds"])):
            p0, p1 = int(block["point_offset"][w]), int(block["point_offset"][w + 1])
            owner = {int(s): j for j, s in enumerate(block["slot_of_point"][p0:p1])}
            assert block["status"][w] == LR.OK or not owner
            named = {}
            for s, o in enumerate(d["origin"][w].tolist()):
                j = owner.get(o, -1) if 0 <= o < d["old_cap"] else -1
                what = (d["seed"], d["index"], w, s)
                assert carry["point"][w, s] == j, what
                assert carry["xyz"][w, s].tobytes() == (src[p0 + j] if j >= 0 else np.zeros(3)).tobytes(), what
                origins.add("-1" if o == -1 else "negative" if o < 0 else "beyond the old capacity" if o >= d["old_cap"]
                            else "an old slot with a landmark" if j >= 0 else "an old slot without a landmark")
                if j >= 0 and o in named:
                    origins.add("two new slots naming one old slot")
                named[o] = s
            assert carry["count"][w] == (carry["point"][w] >= 0).sum()
            slots, carried = slots + d["cap"], carried + int(carry["count"][w])
        seen, px = d["seen"], d["tracks"]
        live = np.arange(d["W"])[None, None, :] < seen[..., None]
        for name, m in (("seen of 0", seen == 0), ("seen above window_len", seen > d["W"]),
                        ("a live pixel that is not finite", (~np.isfinite(px).all(-1) & live).any(-1))):
            if (m & (carry["point"] >= 0)).any():
                origins.add(name)
        rec = loc["records"]
        status |= {int(v) for v in rec["status"].ravel()}
        wstatus |= {int(v) for v in loc["window_status"]}
        ransac_classes(rec, d["params"]["max_iters"], stops)
        size_classes(rec, d["cap"], sizes)
        bad = rec["status"] != PS.OK
        assert not rec["pose6"][bad].any() and not rec["inliers"][bad].any() and not loc["mask"][bad].any()
        # a window whose frames 0 and 1 are OK but a later one is not keeps the pose before: rule E
        for w in np.flatnonzero(loc["window_status"] == S.CR.CARRY_OK):
            for k in np.flatnonzero(bad[w]):
                stops.add("a frame that keeps the pose before it")
                assert loc["poses6"][w, k].tobytes() == loc["poses6"][w, k - 1].tobytes()
    want = {"-1", "negative", "beyond the old capacity", "an old slot with a landmark", "an old slot without a landmark",
            "two new slots naming one old slot", "seen of 0", "seen above window_len", "a live pixel that is not finite"}
    assert origins >= want, want - origins
    assert old_status == {LR.OK, LR.BASELINE, LR.EMPTY, LR.BAD_POSE}, old_status
    assert status == {PS.OK, PS.SKIPPED, PS.FEW_POINTS, PS.NO_MODEL}, status
    assert wstatus == {S.CR.CARRY_OK, S.CR.CARRY_LOST}
    assert stops >= RANSAC_WANT | {"a frame that keeps the pose before it"}, stops
    assert sizes >= SIZE_WANT, SIZE_WANT - sizes
    print("carry: %d draws, %d windows, %d new slots of which %d carried, old status %s, origins and tracks %s, record "
          "status %s, window status %s, classes %s; the join == a dictionary look-up on every slot (worst difference 0)"
          % (len(ds), sum(len(d["kinds"]) for d in ds), slots, carried, sorted(old_status), sorted(origins),
             sorted(status), sorted(wstatus), sorted(stops | sizes)))


def plain_describe(img, points, level0_kind, seen, seen_min, count):
    """Rules A-E without reassoc_ref.describe_points: the level-0 image from the oracle's whole-image blurs, the pixel
    by Python's round (ties to even), the state by plain comparisons; then the oracle at every OK pixel of the frame."""
    h, w = img.shape
    level0 = {"copy": lambda a: a, "sep16": O.blur5_sep, "k273": O.blur5_273}[level0_kind](np.ascontiguousarray(img))
    state, pix = [], []
    for s, (x, y) in enumerate(points.tolist()):
        gated = (count is not None and s >= count) or (seen is not None and seen[s] < seen_min)
        if gated or not (math.isfinite(x) and math.isfinite(y) and 0 <= x <= w - 1 and 0 <= y <= h - 1):
            state.append(RR.PD_NONE)
            continue
        X, Y = round(x), round(y)
        inside = S.PD_R <= X <= w - 1 - S.PD_R and S.PD_R <= Y <= h - 1 - S.PD_R
        state.append(RR.PD_OK if inside else RR.PD_BORDER)
        if inside:
            pix.append((X, Y))
    return np.array(state, np.int32), np.array(pix, np.int32).reshape(-1, 2), level0


def test_reloc_classes_and_restatements_against_the_oracle():
    ds = draws("reloc")
    assert {d["frames"].shape[2] for d in ds} == set(S.RELOC_WIDTHS) == \
        {41, 42, 43, 63, 64, 65, 66, 67, 127, 128, 129, 157, 158, 159, 160}
    assert {d["frames"].shape[1] for d in ds} == set(S.RELOC_HEIGHTS) == {41, 47, 48, 49, 63, 64, 65, 160}
    assert {d["frames"].shape[0] for d in ds} == {1, 2, 3, 4}
    assert any(d["frames"].shape[1:] != (160, 160) for d in ds)  # below the context's maximum
    assert {d["row_stride"] > d["frames"].shape[2] for d in ds} == {False, True}
    for bank in (0, 1):
        bs = [d["banks"][bank] for d in ds]
        assert {b["points"].shape[1] for b in bs} == set(S.RELOC_SLOTS) == {1, 3, 4, 5, 255, 256, 257, 513}
        assert {b["layout"] for b in bs} == {"pairs", "lk"}
        assert any(b["seen"] is None for b in bs) and {b["seen_min"] for b in bs} == {0, 1, 2, 3, 4}
        assert any(b["counts"] is None for b in bs)
        cs = [(int(c), b["points"].shape[1]) for b in bs if b["counts"] is not None for c in b["counts"]]
        assert any(c == 0 for c, _ in cs) and any(c == cap for c, cap in cs) and any(0 < c < cap for c, cap in cs)
    used = {d["context"] for d in ds}
    assert {S.RELOC_LEVEL0[i] for i in used} == {"copy", "sep16", "k273"}
    assert {S.RELOC_CONTEXTS[i]["patch_size"] for i in used} == {1, 9, 15, 31, 41}
    # the re-association
    ras = [d["ra"] for d in ds]
    for k in ("qstate", "tstate"):
        assert {r[k].shape[1] for r in ras if r["input"] != "banks"} == set(S.RA_CAPS) == {1, 2, 255, 256, 257, 512, 513}
    both = sum(r["qstate"].shape[1] in S.RA_CAPS and r["tstate"].shape[1] in S.RA_CAPS for r in ras)
    assert both >= len(ds) // 10
    assert {r["qstate"].shape[0] for r in ras} == {1, 2, 3, 4}
    assert {r["kind"] for r in ras} == set(S.RA_KINDS) | {"described"}
    assert {r["input"] for r in ras} == set(S.RA_INPUTS)
    assert {r["ratio"] for r in ras} == {0.7, 0.8, 1.0} and {r["max_distance"] for r in ras} == {0, 40, 256}
    assert {r["unique"] for r in ras} == {0, 1}
    special = set()
    for d in ds:
        for b in d["banks"]:
            p = b["points"].reshape(-1, 2)
            with np.errstate(invalid="ignore"):
                frac = p - np.floor(p)
                for name, m in (("NaN", np.isnan(p).any(1)), ("+inf", (p == np.inf).any(1)), ("-inf", (p == -np.inf).any(1)),
                                ("negative", (p < 0).any(1)), ("-0.0", ((p == 0) & np.signbit(p)).any(1)),
                                (".5 tie to an even pixel", ((frac == 0.5) & (np.floor(p) % 2 == 0)).any(1)),
                                (".5 tie to an odd pixel", ((frac == 0.5) & (np.floor(p) % 2 == 1)).any(1))):
                    if m.any():
                        special.add(name)
    want = {"NaN", "+inf", "-inf", "negative", "-0.0", ".5 tie to an even pixel", ".5 tie to an odd pixel"}
    assert special >= want, want - special
    # rules A-E: every state in every kind of level-0 image, R and R - 1 from every border, and the restatement's
    # OK slots against the oracle on the whole frame
    states, borders = set(), set()
    frames = ok_slots = 0
    big = False
    for d in ds:
        kind = S.RELOC_LEVEL0[d["context"]]
        patch = S.RELOC_CONTEXTS[d["context"]]["patch_size"]
        nf, h, w = d["frames"].shape
        for b, e in zip(d["banks"], d["expected"]["banks"]):
            for f in range(nf):
                what = (d["seed"], d["index"], f)
                state, pix, level0 = plain_describe(d["frames"][f], b["points"][f], kind,
                                                    None if b["seen"] is None else b["seen"][f], b["seen_min"],
                                                    None if b["counts"] is None else int(b["counts"][f]))
                assert state.tolist() == e["state"][f].tolist(), what
                ok = state == RR.PD_OK
                assert e["n_ok"][f] == ok.sum() and np.array_equal(b["pix"][f][ok], pix), what
                angle = O.orientations(level0, pix, patch)
                desc = O.brief(level0, pix, angle)[0]
                assert e["desc"][f][ok].tobytes() == desc.tobytes(), what
                assert np.array_equal(S.bits(e["angle"][f][ok]), S.bits(angle)), what
                assert not e["desc"][f][~ok].any() and not S.bits(e["angle"][f])[~ok].any(), what
                states |= {(kind, int(s)) for s in np.unique(state)}
                big = big or e["n_ok"][f] > 256
                for name, m in (("x == R", pix[:, 0] == S.PD_R), ("x == w - 1 - R", pix[:, 0] == w - 1 - S.PD_R),
                                ("y == R", pix[:, 1] == S.PD_R), ("y == h - 1 - R", pix[:, 1] == h - 1 - S.PD_R)):
                    if m.any():
                        borders.add(name)
                live = state != RR.PD_NONE
                px = b["pix"][f]
                for name, m in (("x == R - 1", px[:, 0] == S.PD_R - 1), ("x == w - R", px[:, 0] == w - S.PD_R),
                                ("y == R - 1", px[:, 1] == S.PD_R - 1), ("y == h - R", px[:, 1] == h - S.PD_R)):
                    if (m & live).any():
                        borders.add(name)
                        assert (state[m & live] == RR.PD_BORDER).all(), what
                frames, ok_slots = frames + 1, ok_slots + int(ok.sum())
    assert states == {(k, s) for k in ("copy", "sep16", "k273") for s in (RR.PD_NONE, RR.PD_BORDER, RR.PD_OK)}, states
    assert len(borders) == 8, borders
    assert big  # n_ok > 256 in some frame: k_pd_classify carries its base into a second chunk with OK slots behind it
    # rules F-J: rule G against the oracle's knn2 on the compacted OK sets, as tests/test_reassoc_ref.py does; the
    # classes of the accepted queries
    found = set()
    windows = queries = accepted = 0
    for d in ds:
        r, e = d["ra"], d["expected"]["ra"]
        for w in range(len(r["qstate"])):
            qd, qs, td, ts = (r[k][w] for k in ("qdesc", "qstate", "tdesc", "tstate"))
            okq, okt = np.flatnonzero(qs == RR.PD_OK), np.flatnonzero(ts == RR.PD_OK)
            idx, dist = O.knn2(qd[okq], td[okt]) if len(okt) else (np.full((len(okq), 2), -1), np.full((len(okq), 2), -1))
            two = idx[:, 1] >= 0
            d1, d2 = dist[:, 0].astype(np.float32).astype(np.float64), dist[:, 1].astype(np.float32).astype(np.float64)
            passed = two & (d1 < r["ratio"] * d2) & (dist[:, 0] <= r["max_distance"])
            origin = np.full(len(qs), -1, np.int64)
            if len(okt):
                origin[okq[passed]] = okt[idx[passed, 0]]
            dd = np.full(len(qs), -1, np.int64)
            dd[okq[passed]] = dist[passed, 0]
            what = (d["seed"], d["index"], w)
            if r["unique"]:  # rule I, written out on the oracle's neighbours: the smallest d1, then the lowest slot
                for t in np.unique(origin[origin >= 0]):
                    qs_t = np.flatnonzero(origin == t)
                    keep = qs_t[np.lexsort((qs_t, dd[qs_t]))[0]]
                    tie = qs_t[dd[qs_t] == dd[keep]]
                    if len(tie) > 1 and len(set((tie // 256).tolist())) > 1:
                        found.add("a unique tie between queries of different 256-blocks")
                    if len(qs_t) > 1 and dd[qs_t].min() < dd[qs_t].max():
                        found.add("a train slot kept by the nearer query")
                    lose = qs_t[qs_t != keep]
                    origin[lose], dd[lose] = -1, -1
            assert np.array_equal(e["origin"][w], origin) and np.array_equal(e["dist"][w], dd), what
            assert e["count"][w] == (origin >= 0).sum(), what
            if (origin[256:] >= 0).any():
                found.add("accepted queries at slots >= 256")
            if (origin >= 256).any():
                found.add("accepted train slots >= 256")
            if (two & (dist[:, 0] == dist[:, 1])).any():
                found.add("d1 == d2")
            if len(okt) == 1:
                found.add("one OK train slot")
            if len(okt) == 0:
                found.add("no OK train slot")
            if r["input"] == "banks" and (origin >= 0).any():
                found.add("matches between the two banks")
            windows, queries, accepted = windows + 1, queries + len(qs), accepted + int((origin >= 0).sum())
    want = {"a unique tie between queries of different 256-blocks", "a train slot kept by the nearer query",
            "accepted queries at slots >= 256", "accepted train slots >= 256", "d1 == d2", "one OK train slot",
            "no OK train slot", "matches between the two banks"}
    assert found >= want, want - found
    print("reloc: %d draws; described %d frames, %d OK slots, every state on every level-0 kind, borders %s, points %s; "
          "re-associated %d windows, %d queries, %d accepted, classes %s; rules A-E == the oracle on the whole frame "
          "and rules F-J == the oracle's knn2 on the compacted sets, on all (worst difference 0)" % (
              len(ds), frames, ok_slots, sorted(borders), sorted(special), windows, queries, accepted, sorted(found)))
