"""CPU-only: tests/reassoc_ref.py, the numpy restatement of the re-association (DESIGN.md §9 rank 19 rules F-J), pinned
where something independent exists -- rule G against the oracle's oracle_knn2 on the compacted OK sets -- and checked on
the cases the synthetic windows are there for: duplicated train descriptors (d1 == d2, the ratio fails), identical
queries (the unique tie goes to the lowest slot), a train set with one OK slot (no second neighbour), an empty one."""
import numpy as np
import pytest

import oracle_lib as O
import reassoc_ref as R


@pytest.fixture(scope="module")
def sets():
    return R.synthetic_windows()


def test_rule_g_is_the_oracles_knn2_on_the_compacted_ok_sets(sets):
    qdesc, qstate, tdesc, tstate = sets
    for w in range(3):
        okq, okt = np.flatnonzero(qstate[w] == R.PD_OK), np.flatnonzero(tstate[w] == R.PD_OK)
        nn = R.knn2_slots(qdesc[w], qstate[w], tdesc[w], tstate[w])
        assert (nn[np.setdiff1d(np.arange(len(qstate[w])), okq)] == -1).all()  # rule F on the query side
        if len(okt) == 0:
            assert (nn == -1).all()
            continue
        idx, dist = O.knn2(qdesc[w][okq], tdesc[w][okt])
        for i, q in enumerate(okq):
            assert nn[q, 0] == okt[idx[i, 0]] and nn[q, 1] == dist[i, 0], (w, q)
            if len(okt) > 1:
                assert nn[q, 2] == okt[idx[i, 1]] and nn[q, 3] == dist[i, 1], (w, q)
            else:
                assert idx[i, 1] == -1 and nn[q, 2] == -1 and nn[q, 3] == -1


def test_the_cases_are_what_they_are_there_for(sets):
    qdesc, qstate, tdesc, tstate = sets
    nn = R.knn2_slots(qdesc[0], qstate[0], tdesc[0], tstate[0])
    plain = R.reassociate(qdesc, qstate, tdesc, tstate, 0.8, 256, 0)
    uniq = R.reassociate(qdesc, qstate, tdesc, tstate, 0.8, 256, 1)
    # the duplicated train descriptor: both neighbours at the same distance, the lower slot first, the ratio fails
    assert tuple(nn[0]) == (7, 3, 201, 3) and plain["origin"][0, 0] == -1 and plain["dist"][0, 0] == -1
    # identical queries: both accepted without `unique`, the lowest slot keeps the train slot with it
    assert plain["origin"][0, 3] == plain["origin"][0, 40] == 12 and plain["dist"][0, 3] == plain["dist"][0, 40] == 5
    assert uniq["origin"][0, 3] == 12 and uniq["origin"][0, 40] == -1 and uniq["dist"][0, 40] == -1
    # two queries of one train slot at different distances: the nearer one keeps it, although its slot is higher
    assert plain["origin"][0, 5] == plain["origin"][0, 6] == 30 and (plain["dist"][0, 5], plain["dist"][0, 6]) == (4, 2)
    assert uniq["origin"][0, 5] == -1 and uniq["origin"][0, 6] == 30
    # rule F: a train slot that is not OK is never matched, a query that is not OK matches nothing
    assert (tstate[0][plain["origin"][0][plain["origin"][0] >= 0]] == R.PD_OK).all()
    assert nn[8, 1] > 60  # (its exact copy is a slot that does not take part)
    assert (plain["origin"][0, [10, 11]] == -1).all()
    # the counts; `unique` only ever rejects
    assert plain["count"][0] == (plain["origin"][0] >= 0).sum() > uniq["count"][0] > 20
    assert ((uniq["origin"] == plain["origin"]) | (uniq["origin"] == -1)).all()
    kept = uniq["origin"][0][uniq["origin"][0] >= 0]
    assert len(set(kept.tolist())) == len(kept)
    # one OK train slot: a first neighbour at distance 0, no second one, no match; no OK train slot: nothing at all
    nn1 = R.knn2_slots(qdesc[1], qstate[1], tdesc[1], tstate[1])
    assert tuple(nn1[0]) == (123, 0, -1, -1) and (plain["origin"][1:] == -1).all() and (plain["dist"][1:] == -1).all()
    assert plain["count"].tolist()[1:] == [0, 0] == uniq["count"].tolist()[1:]


def test_ratio_and_distance_gates(sets):
    qdesc, qstate, tdesc, tstate = sets
    nn = R.knn2_slots(qdesc[0], qstate[0], tdesc[0], tstate[0])
    for ratio, maxd in ((0.8, 40), (1.0, 256), (1.0, 40), (0.0, 256)):
        got = R.reassociate_window(qdesc[0], qstate[0], tdesc[0], tstate[0], ratio, maxd, 0)[0]
        want = (nn[:, 2] >= 0) & (nn[:, 1].astype(np.float64) < ratio * nn[:, 3].astype(np.float64)) & (nn[:, 1] <= maxd)
        assert np.array_equal(got >= 0, want) and np.array_equal(got[want], nn[want, 0])
    # ratio 1.0 still rejects d1 == d2; max_distance 40 rejects what the ratio alone accepts
    assert R.reassociate_window(qdesc[0], qstate[0], tdesc[0], tstate[0], 1.0, 256, 0)[0][0] == -1
    a = R.reassociate_window(qdesc[0], qstate[0], tdesc[0], tstate[0], 0.8, 256, 0)[2]
    b = R.reassociate_window(qdesc[0], qstate[0], tdesc[0], tstate[0], 0.8, 40, 0)[2]
    assert a > b > 0


def test_empty_sets():
    z = np.zeros((0, 32), np.uint8)
    s = np.zeros(0, np.int32)
    one = np.zeros((1, 32), np.uint8)
    assert R.reassociate_window(z, s, z, s)[2] == 0
    o, d, c = R.reassociate_window(one, np.array([R.PD_OK]), z, s)
    assert o.tolist() == [-1] and d.tolist() == [-1] and c == 0
    assert R.reassociate_window(z, s, one, np.array([R.PD_OK]))[2] == 0
