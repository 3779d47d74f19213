"""Node-pair scores from a plan's resident baskets (GrankPlan.pairs / pair_scores; include/ppr_hip.h
ppr_grank_plan_pairs) against the definition restated in Python from the fetched slab: fwd / bwd are
the rows' own scores, rank the position by (score desc, key asc), common the size of the key
intersection, dot the sum of floor(fl(a * b) * 2^93) over the common keys in Python integers, rounded
once. fwd, bwd and dot are compared as bit patterns, everything else as integers."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

import test_gpu_sweep as sweep_tests  # (its graph families)

pytestmark = pytest.mark.gpu

ARG, RANGE, SOURCE = 1, 11, 12
ALL = ("fwd", "bwd", "rank", "common", "dot")
LOOK = ("fwd", "bwd", "rank")
OUT_BYTES = {"fwd": 8, "bwd": 8, "rank": 4, "common": 4, "dot": 8}


def hash_b(keys):
    """the row order's hash (csrc/ppr_device.h hash_b), all 32 bits"""
    x = (np.asarray(keys, dtype=np.uint64) ^ np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_dot_term_is_the_fraction_floor():
    """the oracle's integer term is the definition's int(Fraction(a * b) * 2**93)"""
    rng = np.random.default_rng(0)
    for a, b in zip(rng.random(2000) * 2.0 ** rng.integers(-60, 1, 2000), rng.random(2000)):
        p = float(a) * float(b)
        n, d = p.as_integer_ratio()
        assert (n << 93) // d == int(Fraction(p) * 2**93)


# ---- the definition -----------------------------------------------------------------------------
class Oracle:
    """rows, ranks and segment sizes of a fetched slab; a row's tables are built once"""

    def __init__(self, slab):
        self.ids, self.sc, self.lens = slab
        self.n = len(self.lens)
        self._row, self._rank, self._seg = {}, {}, {}

    def row(self, u):
        if u not in self._row:
            k = int(self.lens[u])
            self._row[u] = dict(zip(self.ids[u, :k].tolist(), self.sc[u, :k].tolist()))
        return self._row[u]

    def rank(self, u):
        if u not in self._rank:
            order = sorted(self.row(u).items(), key=lambda e: (-e[1], e[0]))
            self._rank[u] = {k: i for i, (k, _) in enumerate(order)}
        return self._rank[u]

    def seg(self, u):
        """entries of row u per hash range (the 64 segments of the stored row)"""
        if u not in self._seg:
            k = int(self.lens[u])
            self._seg[u] = np.bincount((hash_b(self.ids[u, :k]) >> np.uint64(26)).astype(np.int64), minlength=64)
        return self._seg[u]

    def dot(self, u, v):
        """(exact dot, the naive fp64 sum in v's fetched order). A term is int(Fraction(p) * 2**93) for the
        fp64 product p = n / d (d a power of two): (n << 93) // d, the same integer without the Fraction."""
        a, b = self.row(u), self.row(v)
        X, naive = 0, 0.0
        for k, s in b.items():
            if k in a:
                p = a[k] * s
                n, d = p.as_integer_ratio()
                X += (n << 93) // d
                naive += p
        return float(Fraction(X, 2**93)), naive

    def pairs(self, gptr, src, cands):
        P = len(cands)
        o = dict(fwd=np.zeros(P), bwd=np.zeros(P), hit=np.zeros(P, np.uint8), rank=np.full(P, -1, np.int32),
                 common=np.zeros(P, np.int32), dot=np.zeros(P), naive=np.zeros(P), cand_len=np.zeros(P, np.int32),
                 src_len=np.array([len(self.row(int(u))) for u in src], dtype=np.int32))
        memo = {}
        for q, u in enumerate(src):
            u = int(u)
            ru, rk = self.row(u), self.rank(u)
            for j in range(int(gptr[q]), int(gptr[q + 1])):
                v = int(cands[j])
                if (u, v) not in memo:
                    rv = self.row(v)
                    memo[(u, v)] = (ru.get(v, 0.0), rv.get(u, 0.0), (1 if v in ru else 0) | (2 if u in rv else 0), rk.get(v, -1),
                                    len(ru.keys() & rv.keys()), len(rv)) + self.dot(u, v)
                (o["fwd"][j], o["bwd"][j], o["hit"][j], o["rank"][j], o["common"][j], o["cand_len"][j], o["dot"][j],
                 o["naive"][j]) = memo[(u, v)]
        return o

    def algo_bytes(self, gptr, src, cands, want, what, overlap, tasks=None):
        """the header's formula from the oracle's counts (default knobs: one task per group with candidates)"""
        Q, P = len(src), len(cands)
        ncand = np.diff(gptr)
        lu = np.array([int(self.lens[int(u)]) for u in src], dtype=np.int64)
        lv = np.array([int(self.lens[int(v)]) for v in cands], dtype=np.int64)
        per_pair = sum(OUT_BYTES[w] for w in what) + 1 + 4  # + hit + cand_len
        b = P * (per_pair + 4) + Q * (4 + 4) + 4 * int(lu.sum())
        if overlap:
            t = (ncand > 0).astype(np.int64) if tasks is None else tasks
            te = int((lu * t).sum())
            b += 12 * te + 128 * int(t.sum()) + (2 * te if "rank" in what else 0)
            b += 4 * int(lv.sum()) + (8 * int(want["common"].sum()) if "dot" in what else 0)
        else:
            segs = 0
            for q, u in enumerate(src):
                for j in range(int(gptr[q]), int(gptr[q + 1])):
                    v = int(cands[j])
                    segs += int(self.seg(int(u))[int(hash_b([v])[0]) >> 26]) + int(self.seg(v)[int(hash_b([int(u)])[0]) >> 26])
            hits = int((want["hit"] & 1).sum()) + int((want["hit"] >> 1).sum())
            b += P * 12 + 4 * segs + 8 * hits + 4 * int(lv.sum())
            if "rank" in what:
                b += 14 * int(lu.sum()) + 128 * Q + 2 * int((want["hit"] & 1).sum())
        return b


def check(res, want, what=ALL):
    assert np.array_equal(res.hit, want["hit"])
    assert np.array_equal(res.src_len, want["src_len"]) and np.array_equal(res.cand_len, want["cand_len"])
    for f in ("fwd", "bwd", "dot"):
        if f in what:
            assert np.array_equal(bits(getattr(res, f)), bits(want[f])), f
        else:
            assert getattr(res, f) is None
    for f in ("rank", "common"):
        if f in what:
            assert getattr(res, f).dtype == np.int32 and np.array_equal(getattr(res, f), want[f]), f
        else:
            assert getattr(res, f) is None


def same(a, b, what=ALL):
    assert np.array_equal(a.hit, b.hit) and np.array_equal(a.src_len, b.src_len) and np.array_equal(a.cand_len, b.cand_len)
    for f in what:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y), f


def pair_set(g, slab, rng):
    """the groups of the definition test, as lists: 60 random sources, each against its first 8 row keys
    in fetched order, the first 8 sources (ascending) whose rows hold it, 8 random nodes and itself; then
    a dangling node as source and as candidate, an empty group, a repeated group, repeated candidates"""
    ids, sc, lens = slab
    n = g.n
    holders = [[] for _ in range(n)]
    for u in range(n):
        for k in ids[u, :lens[u]].tolist():
            holders[k].append(u)
    sources = [int(u) for u in rng.integers(0, n, size=60)]
    groups = []
    for u in sources:
        groups.append(ids[u, :lens[u]][:8].tolist() + holders[u][:8] + [int(v) for v in rng.integers(0, n, size=8)] + [u])
    dang = np.flatnonzero(np.diff(g.row_ptr) == 0)
    if len(dang):  # (rmat10 and sparse600 have some; every node of multi500 and layered16 has successors)
        d = int(dang[0])
        sources.append(d)
        groups.append(holders[d][:6] + [d, sources[0]])
        groups[0].append(d)
    sources.append(sources[1])
    groups.append([])                     # an empty group
    sources.append(sources[2])
    groups.append(list(groups[2]))        # a repeated group
    sources.append(sources[3])
    groups.append([groups[3][0]] * 5 + groups[3][:4] + [sources[3]] * 2)   # repeated candidates
    return sources, groups


def csr_of(sources, groups):
    gptr = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in groups], out=gptr[1:])
    cands = np.array([v for c in groups for v in c], dtype=np.int32)
    return gptr, np.array(sources, dtype=np.int32), cands


# ---- the plans ----------------------------------------------------------------------------------
GRAPHS = sweep_tests.GRAPHS
_plans = {}


def plan_of(name):
    if name not in _plans:
        make, K, L, it = GRAPHS[name]
        g = make()
        plan = ppr.GrankPlan(g, K, L, 0.85)
        plan.run(it, -1.0)
        slab = plan.fetch_slab()
        orc = Oracle(slab)
        sources, groups = pair_set(g, slab, np.random.default_rng(3))
        gptr, src, cands = csr_of(sources, groups)
        _plans[name] = (g, plan, slab, orc, (gptr, src, cands), orc.pairs(gptr, src, cands))
    return _plans[name]


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for entry in _plans.values():
        entry[1].close()
    _plans.clear()


def premises(want):
    assert int((want["common"] >= 2).sum()) >= 500
    assert int((want["hit"] & 1).sum()) >= 300 and int((want["hit"] >> 1).sum()) >= 300
    assert int((bits(want["dot"]) != bits(want["naive"])).sum()) >= 200


# ---- 3. the definition --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_definition(name):
    g, plan, slab, orc, (gptr, src, cands), want = plan_of(name)
    premises(want)
    assert np.any(np.diff(gptr) == 0) and len(set(src.tolist())) < len(src)
    if name in ("rmat10", "sparse600"):
        d = int(np.flatnonzero(np.diff(g.row_ptr) == 0)[0])
        assert d in src.tolist() and d in cands.tolist() and slab[2][d] == 1
    Q, P = len(src), len(cands)
    for what, overlap in ((ALL, True), (LOOK, False), (("fwd",), False), (("common",), True), (("dot", "rank"), True)):
        st = {}
        res = plan.pairs(src, (gptr, cands), what=what, stats=st)
        check(res, want, what)
        assert np.array_equal(res.gptr, gptr) and np.array_equal(res.sources, src) and np.array_equal(res.candidates, cands)
        assert (st["pairs"], st["groups"]) == (P, Q) and st["lookup_pairs"] + st["overlap_pairs"] == P
        assert st["overlap_pairs"] == (P if overlap else 0)
        assert st["algo_bytes"] == orc.algo_bytes(gptr, src, cands, want, what, overlap), what
        tiers = st["wave_groups"] + st["wg_groups"] + st["split_groups"]
        assert tiers == (Q if overlap else 0) and st["chunks"] == 1 and st["device_ms"] > 0
    # the list-of-lists form and the flat form give the same numbers
    groups = [cands[gptr[q]:gptr[q + 1]].tolist() for q in range(Q)]
    same(plan.pairs(src.tolist(), groups), plan.pairs(src, (gptr, cands)))
    flat_u = np.repeat(src, np.diff(gptr))
    perm = np.random.default_rng(5).permutation(P)
    fl = plan.pair_scores(flat_u[perm], cands[perm])
    assert np.array_equal(fl.sources, flat_u[perm]) and np.array_equal(fl.candidates, cands[perm])
    for f in ("fwd", "bwd", "dot"):
        assert np.array_equal(bits(getattr(fl, f)), bits(want[f][perm])), f
    for f in ("rank", "common", "hit", "cand_len"):
        assert np.array_equal(getattr(fl, f), want[f][perm]), f
    assert np.array_equal(fl.src_len, np.repeat(want["src_len"], np.diff(gptr))[perm])
    # Jaccard from the counts
    r = plan.pairs(src, (gptr, cands), what=("common",))
    den = r.pair_src_len + r.cand_len - r.common
    assert np.all(den > 0) and np.array_equal(r.jaccard(), r.common / den)


# ---- 4. tier, split, chunk and order independence -----------------------------------------------
def test_tier_split_chunk_order_independence(monkeypatch):
    g, plan, slab, orc, (gptr, src, cands), want = plan_of("rmat10")
    Q, P = len(src), len(cands)
    ncand = np.diff(gptr)
    assert ncand.max() > 16 and (ncand > 3).sum() > 50 and (ncand <= 3).sum() >= 1
    st = {}
    base = plan.pairs(src, (gptr, cands), stats=st)
    check(base, want)
    assert st["wave_groups"] == int((ncand <= 16).sum()) and st["wg_groups"] == int((ncand > 16).sum()) and st["split_groups"] == 0
    big = 1 << 30
    forced = [(dict(PPR_PR_WAVE_MAX=big), dict(wave_groups=Q, wg_groups=0, split_groups=0, chunks=1)),
              (dict(PPR_PR_WAVE_MAX=0), dict(wave_groups=0, wg_groups=Q, split_groups=0, chunks=1)),
              (dict(PPR_PR_SPLIT=3), dict(split_groups=int((ncand > 3).sum()), wg_groups=0, wave_groups=int((ncand <= 3).sum()))),
              (dict(PPR_PR_SPLIT=3, PPR_PR_WAVE_MAX=0), dict(split_groups=int((ncand > 3).sum()), wave_groups=0)),
              (dict(PPR_PR_CHUNK=1), dict(chunks=Q)),
              (dict(PPR_PR_CHUNK=7, PPR_PR_SPLIT=5), dict(chunks=(Q + 6) // 7)),
              (dict(PPR_PR_SEARCH=1), dict()), (dict(PPR_PR_SEARCH=2), dict()),
              (dict(PPR_PR_SEARCH=2, PPR_PR_WAVE_MAX=0, PPR_PR_SPLIT=2), dict())]
    for env, counters in forced:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, str(v))
            st = {}
            same(plan.pairs(src, (gptr, cands), stats=st), base)
            for k, v in counters.items():
                assert st[k] == v, (env, k)
            assert st["wave_groups"] + st["wg_groups"] + st["split_groups"] == Q
            if env.get("PPR_PR_SPLIT") == 3 and "PPR_PR_WAVE_MAX" not in env:
                tasks = (ncand + 2) // 3
                assert st["algo_bytes"] == orc.algo_bytes(gptr, src, cands, want, ALL, True, tasks=tasks)
            # the lookup class is cut into the same chunks
            st = {}
            same(plan.pairs(src, (gptr, cands), what=LOOK, stats=st), base, LOOK)
            if "chunks" in counters:
                assert st["chunks"] == counters["chunks"]
    # groups reversed
    groups = [cands[gptr[q]:gptr[q + 1]] for q in range(Q)]
    rg, rs, rc = csr_of(src[::-1].tolist(), [c.tolist() for c in groups[::-1]])
    for what in (ALL, LOOK):
        rev = plan.pairs(rs, (rg, rc), what=what)
        check(rev, orc.pairs(rg, rs, rc), what)
        for q in (0, 1, Q // 2, Q - 1):
            a, b = slice(rg[Q - 1 - q], rg[Q - q]), slice(gptr[q], gptr[q + 1])
            for f in what:
                assert np.array_equal(bits(getattr(rev, f)[a]) if f in ("fwd", "bwd", "dot") else getattr(rev, f)[a],
                                      bits(getattr(base, f)[b]) if f in ("fwd", "bwd", "dot") else getattr(base, f)[b]), f
    # candidates shuffled within their groups, compared after un-shuffling
    rng = np.random.default_rng(9)
    perm = np.concatenate([gptr[q] + rng.permutation(int(ncand[q])) for q in range(Q)]).astype(np.int64)
    for what in (ALL, LOOK):
        sh = plan.pairs(src, (gptr, cands[perm]), what=what)
        for f in what + ("hit", "cand_len"):
            x, y = getattr(sh, f), getattr(base, f)[perm]
            assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y), f


# ---- 5. the lookup class against the overlap class ----------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_lookup_equals_overlap(name):
    g, plan, slab, orc, (gptr, src, cands), want = plan_of(name)
    st_l, st_o = {}, {}
    look = plan.pairs(src, (gptr, cands), what=LOOK, stats=st_l)
    over = plan.pairs(src, (gptr, cands), what=LOOK + ("dot",), stats=st_o)
    assert st_l["lookup_pairs"] == len(cands) and st_l["overlap_pairs"] == 0
    assert st_o["overlap_pairs"] == len(cands) and st_o["lookup_pairs"] == 0
    same(look, over, LOOK)
    check(look, want, LOOK)


# ---- 6. row shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 100, 129, 512, 4096])
def test_row_shapes(L, monkeypatch):
    scale = 10 if L <= 2 else 9 if L <= 100 else 8
    g = ppr.rmat(scale, seed=7)
    n = g.n
    plan = ppr.GrankPlan(g, min(16, L), L, 0.85)
    plan.run(8, -1.0)
    slab = plan.fetch_slab()
    lens = slab[2]
    if L >= 512:
        assert lens.max() < L and lens.max() > 64    # rows limited by n, not by L
    elif L > 2:
        assert lens.max() == L and (lens < L).sum() > 0 and lens.min() == 1
    if L == 100:
        assert ((lens % 64 != 0) & (lens > 64)).sum() > 0
    orc = Oracle(slab)
    if L >= 63:  # segments of 0, 1 and many entries
        sizes = np.concatenate([orc.seg(u) for u in range(0, n, 17)])
        assert (sizes == 0).sum() > 0 and (sizes == 1).sum() > 0 and sizes.max() >= (2 if L < 512 else 4)
    rng = np.random.default_rng(L)
    fixed = [0, n - 1] + [int(v) for v in rng.integers(0, n, size=26)] + [int(np.argmax(lens)), int(np.argmin(lens))] + [0, n - 1]
    assert len(fixed) == 32
    src = np.arange(n, dtype=np.int32)
    gptr = np.arange(n + 1, dtype=np.int64) * 32
    cands = np.tile(np.array(fixed, dtype=np.int32), n)
    want = orc.pairs(gptr, src, cands)
    assert int((want["hit"] & 1).sum()) > 0 and int((want["hit"] >> 1).sum()) > 0
    base = plan.pairs(src, (gptr, cands))
    check(base, want)
    check(plan.pairs(src, (gptr, cands), what=LOOK), want, LOOK)
    for search in (1, 2):
        with monkeypatch.context() as mp:
            mp.setenv("PPR_PR_SEARCH", str(search))
            mp.setenv("PPR_PR_WAVE_MAX", "0" if search == 1 else "64")
            same(plan.pairs(src, (gptr, cands)), base)
    plan.close()


# ---- 7. identities ------------------------------------------------------------------------------
def test_identities():
    g, plan, slab, orc, (gptr, src, cands), want = plan_of("rmat10")
    n, K = g.n, plan.K
    u = np.repeat(src, np.diff(gptr))
    ab = plan.pair_scores(u, cands)
    ba = plan.pair_scores(cands, u)
    assert np.array_equal(bits(ab.dot), bits(ba.dot)) and np.array_equal(ab.common, ba.common)
    assert np.array_equal(bits(ab.bwd), bits(ba.fwd)) and np.array_equal(bits(ab.fwd), bits(ba.bwd))
    assert np.array_equal(ab.hit, (ba.hit >> 1) | ((ba.hit & 1) << 1))
    assert int((ab.common > 0).sum()) > 500
    # dot(x, x) is the squared norm: the cosine of a row with itself is 1
    xs = np.unique(u)
    nn = plan.pair_scores(xs, xs, what=("dot", "common"))
    assert np.array_equal(nn.common, nn.src_len) and np.all(nn.cosine(nn.dot, nn.dot) == 1.0)
    # rank < K exactly when v is in the plan's top-K row of u
    top = plan.fetch()
    in_top = np.array([int(v) in top.ids[int(a), :top.lens[int(a)]].tolist() for a, v in zip(u, cands)])
    assert np.array_equal((ab.rank >= 0) & (ab.rank < K), in_top) and in_top.sum() > 300
    ids, sc, lens = slab
    clear = [a for a in range(n) if lens[a] > K and np.sort(sc[a, :lens[a]])[::-1][K - 1] != np.sort(sc[a, :lens[a]])[::-1][K]]
    assert len(clear) > 100
    clear = clear[:100]
    r = plan.pairs(clear, [top.ids[a, :K].tolist() for a in clear], what=("rank", "fwd"))
    assert np.array_equal(r.rank, np.tile(np.arange(K, dtype=np.int32), len(clear)))
    assert np.array_equal(bits(r.fwd), bits(top.scores[clear, :K].reshape(-1)))
    # a column: the sources that hold target t are the hit set of the reverse query
    for t in (int(cands[0]), int(np.argmax(np.bincount(ids[ids >= 0], minlength=n))), int(src[5])):
        col = plan.pairs([t], [list(range(n))], what=("bwd",))       # u = t against every v: bit 1 = t in B[v]
        col2 = plan.pair_scores(np.arange(n), np.full(n, t), what=("fwd",))   # (u, t) over all u: bit 0
        holders = np.flatnonzero(col2.hit & 1)
        assert np.array_equal(holders, np.flatnonzero(col.hit & 2)) and len(holders) > 0
        rq = plan.rquery([[t]], n)
        assert sorted(rq.ids[0, :rq.lens[0]].tolist()) == holders.tolist()
        got = dict(zip(rq.ids[0, :rq.lens[0]].tolist(), rq.scores[0, :rq.lens[0]].tolist()))
        assert all(got[int(a)] == col2.fwd[a] for a in holders)   # (one target of weight 1: the score itself)


# ---- 8. hot-encoded ids -------------------------------------------------------------------------
def test_hot_encoded_ids(monkeypatch):
    for k, v in {"PPR_HOT_N": "64", "PPR_HOT_AT": "1", "PPR_TIER_MASK": "0x20"}.items():
        monkeypatch.setenv(k, v)
    g = ppr.rmat(10, seed=5)
    plan = ppr.GrankPlan(g, 16, 32, 0.85, sum_mode="chain")
    plan.run(6, -1.0)
    raw = np.zeros((g.n, 32), dtype=np.int32)
    rl = np.zeros(g.n, dtype=np.int32)
    hot = 0
    for slot in (0, 1):
        _lib.check(_lib.lib().ppr_plan_fetch_slot(plan._p, slot, _lib.ptr(raw), None, _lib.ptr(rl)))
        hot += sum(int((raw[v, :rl[v]] < 0).sum()) for v in range(g.n))
    assert hot > 0  # the slab does hold tagged ids
    slab = plan.fetch_slab()
    orc = Oracle(slab)
    gptr, src, cands = csr_of(*pair_set(g, slab, np.random.default_rng(3)))
    want = orc.pairs(gptr, src, cands)
    assert int((want["common"] >= 2).sum()) > 0 and int((want["hit"] & 1).sum()) > 0 and int((want["hit"] >> 1).sum()) > 0
    check(plan.pairs(src, (gptr, cands)), want)
    check(plan.pairs(src, (gptr, cands), what=LOOK), want, LOOK)
    monkeypatch.setenv("PPR_PR_WAVE_MAX", "0")
    monkeypatch.setenv("PPR_PR_SEARCH", "2")
    check(plan.pairs(src, (gptr, cands)), want)
    plan.close()


# ---- 9. slots and no trace ----------------------------------------------------------------------
def test_slots_and_no_trace():
    g = ppr.rmat(10, seed=5)
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    rng = np.random.default_rng(2)
    plan.init()
    slab0 = plan.fetch_slab(0)
    u, v = rng.integers(0, g.n, size=300), rng.integers(0, g.n, size=300)
    v[:50] = u[:50]
    gptr, src, cands, _, _ = ppr.normalize_pairs(u, v)
    for what in (ALL, LOOK):
        check(plan.pairs(src, (gptr, cands), what=what, iterations_run=0), Oracle(slab0).pairs(gptr, src, cands), what)
    for it in (1, 3):
        plan.run(it, -1.0)
        slab = plan.fetch_slab()
        gp, s, c = csr_of(*pair_set(g, slab, np.random.default_rng(3)))
        want = Oracle(slab).pairs(gp, s, c)
        check(plan.pairs(s, (gp, c)), want)
        check(plan.pairs(s, (gp, c), what=LOOK), want, LOOK)
    # an earlier iteration count on request
    slab2 = plan.fetch_slab(2)
    check(plan.pairs(s, (gp, c), iterations_run=2), Oracle(slab2).pairs(gp, s, c))
    # the calls left no trace: the next run equals a fresh plan's
    plan.run(6, -1.0)
    fresh = ppr.GrankPlan(g, 16, 32, 0.85)
    fresh.run(6, -1.0)
    a, b = plan.fetch(), fresh.fetch()
    assert np.array_equal(a.ids, b.ids) and np.array_equal(bits(a.scores), bits(b.scores)) and np.array_equal(a.lens, b.lens)
    assert all(np.array_equal(x, y) for x, y in zip(plan.fetch_slab(), fresh.fetch_slab()))
    plan.close()
    fresh.close()


# ---- 10. refusals -------------------------------------------------------------------------------
SENT = -77
OUTS = ("fwd", "bwd", "hit", "rank", "common", "dot", "slen", "clen")


def raw_call(plan, gptr=(0, 2, 3), sources=(1, 2), cands=(3, 4, 5), Q=None, flags=0, p=None, it=None, nulls=(), outs=OUTS):
    """the C call on sentinel-filled outputs; returns (code, outputs)"""
    gp = None if gptr is None else np.ascontiguousarray(gptr, dtype=np.int64)
    src = np.ascontiguousarray(sources, dtype=np.int32)
    cd = np.ascontiguousarray(cands, dtype=np.int32)
    nq = (len(gp) - 1 if gp is not None else len(src)) if Q is None else Q
    dt = dict(fwd=np.float64, bwd=np.float64, hit=np.uint8, rank=np.int32, common=np.int32, dot=np.float64, slen=np.int32,
              clen=np.int32)
    o = {k: np.zeros(max(len(src) if k == "slen" else len(cd), 1), dtype=dt[k]) for k in OUTS}
    for k in o:
        o[k][:] = np.array(SENT).astype(dt[k])  # (the byte 179 in out_hit)
    ptr = {k: (_lib.ptr(o[k]) if k in outs and k not in nulls else None) for k in OUTS}
    rc = _lib.lib().ppr_grank_plan_pairs(
        plan._p if p is None else p, plan.iterations_run if it is None else it, nq, None if gp is None else _lib.ptr(gp),
        None if "sources" in nulls else _lib.ptr(src), None if "cands" in nulls else _lib.ptr(cd), flags,
        *(ptr[k] for k in OUTS), None)
    return rc, o


def untouched(o):
    return all(np.all(v == np.array(SENT).astype(v.dtype)) for v in o.values())


def test_refusals():
    g, plan, slab, orc, (gptr, src, cands), want = plan_of("rmat10")
    n = g.n
    rc, o = raw_call(plan)
    assert rc == 0 and not untouched(o)
    cases = [
        (ARG, dict(p=0)),                                  # a null plan
        (ARG, dict(it=-1)),
        (ARG, dict(gptr=None, Q=2)),
        (ARG, dict(Q=-1)),
        (ARG, dict(gptr=(1, 2, 3))),                       # does not start at 0
        (ARG, dict(gptr=(0, 3, 2))),                       # not monotone
        (ARG, dict(nulls=("sources",))),
        (ARG, dict(nulls=("cands",))),
        (ARG, dict(flags=1)),
        (ARG, dict(flags=1 << 31)),
        (ARG, dict(outs=())),                              # every output pointer NULL
        (RANGE, dict(gptr=(0, 1 << 31), sources=(1,), cands=(3,))),   # P beyond 2^31 - 1, decided before a candidate is read
        (SOURCE, dict(sources=(1, n))),
        (SOURCE, dict(sources=(-1, 2))),
        (SOURCE, dict(cands=(3, n, 5))),
        (SOURCE, dict(cands=(3, 4, -1))),
        # the order when two apply
        (ARG, dict(gptr=(0, 1 << 31), sources=(1,), cands=(3,), flags=2)),   # flags before the range
        (ARG, dict(gptr=(0, 1 << 31), sources=(1,), cands=(3,), outs=())),   # no output before the range
        (ARG, dict(gptr=(0, 1 << 31), sources=(n,), nulls=("cands",))),     # null candidates before the range and the ids
        (RANGE, dict(gptr=(0, 1 << 31), sources=(n,), cands=(3,))),         # the range before the ids
        (ARG, dict(sources=(n, 2), flags=4)),
        (ARG, dict(sources=(n, 2), gptr=(0, 3, 2))),
        (ARG, dict(cands=(n, 4, 5), it=-2)),
    ]
    for code, kw in cases:
        rc, o = raw_call(plan, **kw)
        assert rc == code, kw
        assert untouched(o), kw
    # an MC plan
    mc = ppr.MccpPlan(g, 16, 64, 0.85)
    rc, o = raw_call(plan, p=mc._p)
    assert rc == ARG and untouched(o)
    mc.close()
    # the stats are cleared by a refused call
    st = _lib.PprPairsStats()
    st.pairs = 9
    assert _lib.lib().ppr_grank_plan_pairs(plan._p, plan.iterations_run, -1, None, None, None, 0, None, None, None, None, None,
                                           None, None, None, ctypes.byref(st)) == ARG and st.pairs == 0
    # no group, and groups without candidates: PPR_OK, only out_slen is written
    rc, o = raw_call(plan, gptr=(0,), sources=(), cands=())
    assert rc == 0 and untouched(o)
    rc, o = raw_call(plan, gptr=(0, 0, 0), sources=(5, 6), cands=())
    assert rc == 0 and o["slen"].tolist() == [int(slab[2][5]), int(slab[2][6])]
    assert untouched({k: v for k, v in o.items() if k != "slen"})
    rc, o = raw_call(plan, gptr=(0, 0, 0), sources=(5, 6), cands=(), outs=("fwd", "dot"))
    assert rc == 0 and untouched(o)
    # optional outputs: a NULL one is not written, the others are
    rc, o = raw_call(plan, gptr=gptr, sources=src, cands=cands, outs=("bwd", "common"))
    assert rc == 0 and np.array_equal(bits(o["bwd"]), bits(want["bwd"])) and np.array_equal(o["common"], want["common"])
    assert untouched({k: v for k, v in o.items() if k not in ("bwd", "common")})
    # the Python surface raises with the code, and the plan answers a normal call afterwards
    with pytest.raises(ppr.PprError) as e:
        plan.pairs([n], [[0]])
    assert e.value.code == SOURCE
    with pytest.raises(ppr.PprError) as e:
        plan.pair_scores([0], [-1])
    assert e.value.code == SOURCE
    with pytest.raises(ValueError):
        plan.pairs([0, 1], [[0]])
    with pytest.raises(ValueError):
        plan.pairs([0], [[0]], what=("score",))
    check(plan.pairs(src, (gptr, cands)), want)
    e = plan.pairs([], [])
    assert len(e.hit) == 0 and len(e.src_len) == 0 and e.gptr.tolist() == [0] and e.dot.shape == (0,)
