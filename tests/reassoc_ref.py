"""numpy restatement of the re-association (DESIGN.md §9 rank 19 rules F-J; include/orbx_reloc.h) and of the rules A-E
of the point descriptors on the CPU oracle, plus the synthetic descriptor sets the tests share.  Independent of the
library: plain loops over slots, the Hamming distance from a bit-count table."""
import numpy as np

import oracle_lib as O

PD_NONE, PD_BORDER, PD_OK = 0, 1, 2
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """distance of one 32-byte descriptor to every row of b"""
    return _POP[np.bitwise_xor(np.asarray(a, np.uint8)[None, :], np.asarray(b, np.uint8).reshape(-1, 32))].sum(axis=1)


def knn2_slots(qdesc, qstate, tdesc, tstate):
    """Rules F-G of one window: per query slot (j1, d1, j2, d2) over the OK train slots, -1 where there is none; ties
    keep the lower train slot.  A query that is not OK has none."""
    nq = len(qstate)
    out = np.full((nq, 4), -1, np.int64)
    ok_t = np.flatnonzero(np.asarray(tstate) == PD_OK)
    for q in range(nq):
        if qstate[q] != PD_OK or len(ok_t) == 0:
            continue
        d = hamming(qdesc[q], np.asarray(tdesc)[ok_t])
        order = np.lexsort((ok_t, d))  # by distance, then by slot
        out[q, 0], out[q, 1] = ok_t[order[0]], d[order[0]]
        if len(order) > 1:
            out[q, 2], out[q, 3] = ok_t[order[1]], d[order[1]]
    return out


def reassociate_window(qdesc, qstate, tdesc, tstate, ratio=0.8, max_distance=256, unique=1):
    """Rules F-J of one window: (origin (nq) int32, dist (nq) int32, count)."""
    nn = knn2_slots(qdesc, qstate, tdesc, tstate)
    nq = len(qstate)
    origin, dist = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    for q in range(nq):
        j1, d1, j2, d2 = (int(v) for v in nn[q])
        if j1 < 0 or j2 < 0:
            continue  # rule H: a second neighbour exists
        if float(np.float32(d1)) < ratio * float(np.float32(d2)) and d1 <= max_distance:
            origin[q], dist[q] = j1, d1
    if unique:
        for t in set(origin[origin >= 0].tolist()):
            qs = np.flatnonzero(origin == t)
            keep = min(qs, key=lambda q: (dist[q], q))  # rule I: the smallest d1, then the lowest query slot
            for q in qs:
                if q != keep:
                    origin[q], dist[q] = -1, -1
    return origin, dist, int((origin >= 0).sum())


def reassociate(qdesc, qstate, tdesc, tstate, ratio=0.8, max_distance=256, unique=1):
    """The batch: qdesc (n, qcap, 32), qstate (n, qcap), tdesc (n, tcap, 32), tstate (n, tcap) -> dict of origin, dist
    (n, qcap) int32 and count (n) int32."""
    res = [reassociate_window(qdesc[w], qstate[w], tdesc[w], tstate[w], ratio, max_distance, unique)
           for w in range(len(qdesc))]
    return dict(origin=np.stack([r[0] for r in res]), dist=np.stack([r[1] for r in res]),
                count=np.array([r[2] for r in res], np.int32))


# ---- rules A-E on the oracle ----------------------------------------------------------------------------------------
def pd_radius(patch_size):
    return max(patch_size // 2, 20)


def describe_points(img, points, params, seen=None, seen_min=0, count=None):
    """Rules A-E for one frame: img (h, w) uint8, points (cap, 2) float32, params an oracle_lib.OracleParams.  Returns
    dict of desc (cap, 32) uint8, angle (cap) float32, state (cap) int32, n_ok and, for the tests of rule C, nskip and
    noob of the oracle's BRIEF over the OK slots."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    cap = len(pts)
    R = pd_radius(params.patch_size)
    state, pix = np.zeros(cap, np.int32), np.zeros((cap, 2), np.int32)
    for s in range(cap):
        if count is not None and s >= count:
            continue
        if seen is not None and seen[s] < seen_min:
            continue
        x, y = pts[s]
        if not (np.isfinite(x) and np.isfinite(y) and np.float32(0) <= x <= np.float32(w - 1) and
                np.float32(0) <= y <= np.float32(h - 1)):
            continue
        X, Y = int(np.rint(x)), int(np.rint(y))  # ties to even
        pix[s] = X, Y
        state[s] = PD_OK if R <= X <= w - 1 - R and R <= Y <= h - 1 - R else PD_BORDER
    desc, angle = np.zeros((cap, 32), np.uint8), np.zeros(cap, np.float32)
    ok = np.flatnonzero(state == PD_OK)
    nskip = noob = 0
    if len(ok):
        level0 = O.build_level(img, params, 0)
        a = O.orientations(level0, pix[ok], params.patch_size)
        d, _, nskip, noob = O.brief(level0, pix[ok], a)
        desc[ok], angle[ok] = d, a
    return dict(desc=desc, angle=angle, state=state, n_ok=len(ok), nskip=nskip, noob=noob, pix=pix)


# ---- the synthetic sets of tests/test_reassoc_ref.py and the device parity test --------------------------------------
def flip(desc, rng, nbits):
    """a copy of a 32-byte descriptor with nbits distinct bits flipped"""
    d = np.array(desc, np.uint8)
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def pool_window(rng, qcap, tcap, size=40):
    """One window in the manner of test_matcher.tie_heavy, both sets drawn from a pool of `size` descriptors: (qdesc
    (qcap, 32), tdesc (tcap, 32)).  The first train slots hold distinct pool descriptors, so a query's copy is alone at
    distance 0 and is accepted -- equal queries, of whatever 256-block, tie for that train slot under `unique` --
    unless one of the later train slots (one in twenty holds a pool descriptor, the rest random bytes) repeats it:
    d1 == d2, the ratio fails.  A fifth of the queries have one to three bits flipped: the same train slot at a larger
    distance."""
    pool = rng.integers(0, 256, (size, 32), dtype=np.uint8)
    tdesc = rng.integers(0, 256, (tcap, 32), dtype=np.uint8)
    m = min(size, tcap)
    tdesc[:m] = pool[rng.permutation(size)[:m]]
    rep = np.flatnonzero(rng.random(tcap) < 0.05)
    rep = rep[rep >= m]
    tdesc[rep] = pool[rng.integers(0, size, len(rep))]
    qdesc = pool[rng.integers(0, size, qcap)]
    for q in np.flatnonzero(rng.random(qcap) < 0.2):
        qdesc[q] = flip(qdesc[q], rng, int(rng.integers(1, 4)))
    return qdesc, tdesc


def synthetic_windows(qcap=70, tcap=300, seed=11):
    """Three windows of seeded random 256-bit descriptors: (qdesc (3, qcap, 32), qstate, tdesc (3, tcap, 32), tstate).
    0: 250 OK train slots (others NONE / BORDER with random bytes that must not take part), queries that are copies of
       train slots with 0 .. 60 bits flipped, train slots 7 and 201 identical (d1 == d2: the ratio fails for their
       copies), queries 3 and 40 identical copies of train 12 (the unique tie goes to slot 3), queries 5 and 6 copies
       of train 30 at 4 and 2 flipped bits (6 keeps it), random queries, queries that are not OK
    1: one OK train slot (no second neighbour, no match)
    2: no OK train slot"""
    rng = np.random.default_rng(seed)
    qdesc = rng.integers(0, 256, (3, qcap, 32), dtype=np.uint8)
    tdesc = rng.integers(0, 256, (3, tcap, 32), dtype=np.uint8)
    qstate = np.full((3, qcap), PD_OK, np.int32)
    tstate = np.full((3, tcap), PD_OK, np.int32)
    dead = rng.choice(np.setdiff1d(np.arange(tcap), [7, 12, 30, 201]), tcap - 250, replace=False)
    tstate[0, dead[::2]], tstate[0, dead[1::2]] = PD_NONE, PD_BORDER
    tdesc[0, 201] = tdesc[0, 7]
    live = np.flatnonzero(tstate[0] == PD_OK)
    for q in range(50):
        t = live[(q * 37) % len(live)]
        qdesc[0, q] = flip(tdesc[0, t], rng, (q * 13) % 61)
    qdesc[0, 0] = flip(tdesc[0, 7], rng, 3)       # its twin 201 is as near: d1 == d2
    qdesc[0, 3] = qdesc[0, 40] = flip(tdesc[0, 12], rng, 5)
    qdesc[0, 5], qdesc[0, 6] = flip(tdesc[0, 30], rng, 4), flip(tdesc[0, 30], rng, 2)
    qdesc[0, 8] = tdesc[0, dead[0]]               # an exact copy of a train slot that is not OK
    qstate[0, [10, 11]] = PD_NONE, PD_BORDER      # (copies of live train slots, but not OK themselves)
    tstate[1] = PD_NONE
    tstate[1, 123] = PD_OK
    qdesc[1, 0] = tdesc[1, 123]
    tstate[2] = np.where(np.arange(tcap) % 2, PD_NONE, PD_BORDER)
    return qdesc, qstate, tdesc, tstate
