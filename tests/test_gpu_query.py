"""Preference-set queries (GrankPlan.query / ppr_grank_plan_query) against their definition, restated
with Python integers from the plan's fetched slab: W summed in seed order, f_i = w_i / W,
X[k] = sum floor(fl(s * f_i) * 2^93) over the seeds' baskets, score = X * 2^-93 rounded once, the Kq
best by (score desc, dense id asc). Ids, scores and lens are compared bit for bit, through every
tier (wave, workgroup, key-range split), chunking and query order."""
from fractions import Fraction

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib
from approximated_personalized_pagerank_amd.grank import normalize_queries

pytestmark = pytest.mark.gpu

XS_F = 93
WAVE_MAX, T_MAX = 1536, 8192  # default knobs: wave tier up to 3/4 * 2048 candidates, tables of 8192 slots


# ---- the oracle ---------------------------------------------------------------------------------
def oracle_totals(slab, seeds, weights=None):
    """{key: score} of one query by the definition (exact integers)"""
    ids, sc, lens = slab
    ws = [1.0] * len(seeds) if weights is None else [float(w) for w in weights]
    W = 0.0
    for w in ws:  # in seed order
        W += w
    acc = {}
    for u, w in zip(seeds, ws):
        f = w / W
        u = int(u)
        for j in range(int(lens[u])):
            k = int(ids[u, j])
            acc[k] = acc.get(k, 0) + int(Fraction(float(sc[u, j]) * f) * 2 ** XS_F)
    return {k: float(Fraction(x, 2 ** XS_F)) for k, x in acc.items()}


def oracle_rows(totals, seeds_of, Kq, exclude=False):
    """result arrays of a list of queries from their totals"""
    Q = len(totals)
    ids = np.full((Q, Kq), -1, dtype=np.int32)
    sc = np.zeros((Q, Kq), dtype=np.float64)
    lens = np.zeros(Q, dtype=np.int32)
    for q, t in enumerate(totals):
        drop = set(int(u) for u in seeds_of[q]) if exclude else ()
        top = sorted(((-s, k) for k, s in t.items() if k not in drop))[:Kq]
        lens[q] = len(top)
        for i, (ms, k) in enumerate(top):
            ids[q, i] = k
            sc[q, i] = -ms
    return ids, sc, lens


def same_bits(res, want):
    ids, sc, lens = want
    assert np.array_equal(res.lens, lens)
    assert np.array_equal(res.ids, ids)
    assert np.array_equal(res.scores.view(np.uint64), sc.view(np.uint64))


def cand(lens, seeds):
    return int(sum(int(lens[int(u)]) for u in seeds))


def hash_range(keys):
    """key range of a key: the top 6 bits of the row order's hash (csrc/ppr_device.h hash_b)"""
    x = (np.asarray(keys, dtype=np.uint64) ^ np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(26)).astype(np.int64)


def split_of(slab, seeds, T):
    """the planner's rule restated: the smallest power-of-two split R <= 64 whose every group of 64 / R
    key ranges has at most 3/4 T candidates; None when the fullest single range exceeds that"""
    ids, _, lens = slab
    keys = np.concatenate([ids[int(u), :lens[int(u)]] for u in seeds] + [np.zeros(0, dtype=np.int32)])
    cnt = np.bincount(hash_range(keys), minlength=64)
    for R in (2, 4, 8, 16, 32, 64):
        if cnt.reshape(R, 64 // R).sum(axis=1).max() <= 3 * T // 4:
            return R
    return None


def pick(rng, lens, lo, hi, pool=None):
    """random seeds (distinct) whose candidates C land in [lo, hi]"""
    pool = np.arange(len(lens)) if pool is None else pool
    order = rng.permutation(pool)
    seeds, C = [], 0
    for u in order:
        if C >= lo:
            break
        if C + lens[u] > hi:
            continue
        seeds.append(int(u))
        C += int(lens[u])
    assert lo <= C <= hi, (C, lo, hi)
    return seeds


# ---- the base plan and the mixed query set (tests 1-4) -------------------------------------------
@pytest.fixture(scope="module")
def base():
    g = ppr.rmat(10, seed=5)
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    yield g, plan, slab
    plan.close()


def wave_queries(n, lens, rng):
    dangling = np.nonzero(lens == 1)[0]
    assert len(dangling) > 10
    qs, ws = [[]], [None]                                     # an empty query
    qs.append([int(rng.integers(n))]); ws.append(None)        # a single seed
    qs.append([int(dangling[0]), int(dangling[1]), int(dangling[2])]); ws.append(None)  # dangling seeds only
    qs.append([7, 7, 9, 7]); ws.append([1.0, 2.0, 0.5, 1.0])  # a repeated seed
    qs.append([3, 4, 5]); ws.append([0.0, 1.0, 0.0])          # zero weights
    qs.append([int(dangling[3]), 11]); ws.append([0.0, 3.0])
    while len(qs) < 300:
        k = int(rng.integers(0, 41))
        s = rng.integers(0, n, size=k).tolist()
        mode = len(qs) % 3
        ws.append(None if mode == 0 or k == 0 else
                  (rng.random(k) + 0.01).tolist() if mode == 1 else
                  rng.choice([0.0, 1.0, 2.0, 0.125], size=k).tolist())
        if ws[-1] is not None and sum(ws[-1]) == 0.0:
            ws[-1][0] = 1.0
        qs.append(s)
    return qs, ws


def flat_weights(qs, ws):
    """weights of a query set as one flat array (None rows = 1.0)"""
    return np.concatenate([np.ones(len(q)) if w is None else np.asarray(w, dtype=np.float64)
                           for q, w in zip(qs, ws)] + [np.zeros(0)])


@pytest.fixture(scope="module")
def mixed(base):
    """the query sets of the three tiers and their oracle totals, computed once"""
    g, plan, slab = base
    lens = slab[2]
    rng = np.random.default_rng(11)
    sets = {}
    qs, ws = wave_queries(g.n, lens, rng)
    assert all(cand(lens, q) <= WAVE_MAX for q in qs)
    sets["wave"] = (qs, ws)
    nd = np.nonzero(lens > 1)[0]
    qs = [pick(rng, lens, lo, hi, nd) for lo, hi in [(1950, 2150), (2500, 3000), (4000, 4500), (5800, 6100)]]
    assert all(60 <= len(q) <= 400 for q in qs)
    qs.append(rng.choice(nd, size=150).tolist())              # with repeats
    sets["wg"] = (qs, [None, (rng.random(len(qs[1])) + 0.1).tolist(), None, None, None])
    qs = [rng.integers(0, g.n, size=k).tolist() for k in (300, 520, 777)] + [list(range(g.n))]
    sets["range"] = (qs, [None, None, (rng.random(777) + 0.1).tolist(), None])
    assert cand(lens, qs[-1]) > 3 * T_MAX // 4
    out = {}
    for name, (qs, ws) in sets.items():
        out[name] = (qs, ws, [oracle_totals(slab, q, w) for q, w in zip(qs, ws)])
    return out


def expected_tiers(lens, qs, wave_max=WAVE_MAX, T=T_MAX):
    C = [cand(lens, q) for q in qs]
    wave = sum(c <= wave_max for c in C)
    wg = sum(wave_max < c <= 3 * T // 4 for c in C)
    return wave, wg, len(qs) - wave - wg


def test_wave_tier(base, mixed):
    g, plan, slab = base
    qs, ws, tot = mixed["wave"]
    for Kq in (1, 16, 200):
        res = plan.query(qs, Kq, weights=flat_weights(qs, ws))
        same_bits(res, oracle_rows(tot, qs, Kq))
        assert res.wave_queries == len(qs) and res.wg_queries == 0 and res.range_queries == 0
        assert res.candidates == sum(cand(slab[2], q) for q in qs)
        assert res.algo_bytes == 8 * sum(map(len, qs)) + 12 * res.candidates + len(qs) * (12 * Kq + 4)
    assert res.lens[0] == 0 and (res.lens[1:] < 200).any()  # the empty query; 200 > distinct keys: short rows
    # weights=None: every weight 1.0
    sub = [i for i, w in enumerate(ws) if w is None]
    res = plan.query([qs[i] for i in sub], 16)
    same_bits(res, oracle_rows([tot[i] for i in sub], [qs[i] for i in sub], 16))


def test_workgroup_tier(base, mixed):
    g, plan, slab = base
    qs, ws, tot = mixed["wg"]
    res = plan.query(qs, 16, weights=flat_weights(qs, ws))
    same_bits(res, oracle_rows(tot, qs, 16))
    assert (res.wave_queries, res.wg_queries, res.range_queries) == expected_tiers(slab[2], qs)
    assert res.wg_queries >= 4


@pytest.mark.parametrize("qt", [None, "1024"])
def test_range_tier(base, mixed, monkeypatch, qt):
    g, plan, slab = base
    qs, ws, tot = mixed["range"]
    T = int(qt or T_MAX)
    if qt:
        monkeypatch.setenv("PPR_Q_T", qt)
    R = [split_of(slab, q, T) for q in qs]
    if qt:
        # One key sits in about 800 of the 1024 rows (every RMAT-10 seed tried), so the key range of that
        # key alone holds more than 3/4 * 1024 candidates of a query with that many seeds: by the
        # planner's rule such a query is refused at this table size, and so is a call that holds it.
        assert R[-1] is None and R[0] is not None
        with pytest.raises(ppr.PprError) as e:
            plan.query(qs, 16, weights=flat_weights(qs, ws))
        assert e.value.code == 11
    fit = [i for i, r in enumerate(R) if r is not None]
    assert len(fit) == len(qs) if not qt else len(fit) >= 1
    qs, ws, tot, R = [qs[i] for i in fit], [ws[i] for i in fit], [tot[i] for i in fit], [R[i] for i in fit]
    for Kq in (16, 200):
        res = plan.query(qs, Kq, weights=flat_weights(qs, ws))
        same_bits(res, oracle_rows(tot, qs, Kq))
    assert (res.wave_queries, res.wg_queries, res.range_queries) == expected_tiers(slab[2], qs, T=T)
    assert res.range_queries > 0 and res.max_ranges == max(R) and res.max_ranges >= (16 if qt else 2)


def test_tier_independence(base, mixed, monkeypatch):
    """the same queries through other tiers, chunk sizes, call splits and query orders: identical bits"""
    g, plan, slab = base
    qs = mixed["wave"][0][::4] + mixed["wg"][0] + mixed["range"][0]
    ws = mixed["wave"][1][::4] + mixed["wg"][1] + mixed["range"][1]
    tot = mixed["wave"][2][::4] + mixed["wg"][2] + mixed["range"][2]
    Kq = 16
    want = oracle_rows(tot, qs, Kq)
    Q = len(qs)

    def ask(idx):
        sub, wsub = [qs[i] for i in idx], [ws[i] for i in idx]
        return plan.query(sub, Kq, weights=flat_weights(sub, wsub))

    # (queries whose fullest key range exceeds 3/4 of a 1024-slot table are refused at that size: see
    # test_range_tier; they take part in the other three ways)
    narrow = [i for i in range(Q) if cand(slab[2], qs[i]) <= 768 or split_of(slab, qs[i], 1024) is not None]
    assert Q - len(narrow) <= 3

    for env, split in [({}, False), ({"PPR_Q_WAVE_MAX": "0"}, True), ({"PPR_Q_T": "1024"}, False),
                       ({"PPR_Q_CHUNK": "7"}, True)]:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            idx = narrow if "PPR_Q_T" in env else list(range(Q))
            res = ask(idx)
            same_bits(res, tuple(a[idx] for a in want))
            if env.get("PPR_Q_WAVE_MAX") == "0":
                assert res.wave_queries == 0
            if split:  # two calls, each in reversed query order
                for part in (list(range(Q // 2))[::-1], list(range(Q // 2, Q))[::-1]):
                    r2 = ask(part)
                    same_bits(r2, tuple(a[part] for a in want))


# ---- padded rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,L", [(10, 100), (11, 128)])
def test_padded_rows(scale, L):
    """L = 100 (rows narrower than the kernels' padded width 128) and L = 128 on another graph: one wave,
    one workgroup and one range query each"""
    g = ppr.rmat(scale, seed=5 + scale)
    plan = ppr.GrankPlan(g, 16, L, 0.85)
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    lens = slab[2]
    rng = np.random.default_rng(scale)
    nd = np.nonzero(lens > 1)[0]
    qs = [pick(rng, lens, 300, 1200, nd), pick(rng, lens, 2500, 5500, nd), pick(rng, lens, 12000, 40000)]
    assert expected_tiers(lens, qs) == (1, 1, 1)
    res = plan.query(qs, 50)
    same_bits(res, oracle_rows([oracle_totals(slab, q) for q in qs], qs, 50))
    assert (res.wave_queries, res.wg_queries, res.range_queries) == (1, 1, 1)
    plan.close()


# ---- ties at the cut -----------------------------------------------------------------------------
def twin_graph():
    """two identical components of 96 nodes (ids v and v + 96), about 6 random successors per node,
    every seventh node dangling"""
    rng = np.random.default_rng(3)
    H = 96
    succ = [[] if v % 7 == 0 else sorted(set(rng.integers(0, H, size=6).tolist())) for v in range(H)]
    rows = succ + [[s + H for s in r] for r in succ]
    rp = np.zeros(2 * H + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return ppr.Csr(rp, np.array([s for r in rows for s in r], dtype=np.int32)), H


@pytest.mark.parametrize("tier,env", [("wave", {}), ("wg", {"PPR_Q_WAVE_MAX": "0"}),
                                      ("range", {"PPR_Q_WAVE_MAX": "0", "PPR_Q_T": "256"})])
def test_ties_at_the_cut(tier, env, monkeypatch):
    """every key k of a query {v, v + 96} is tied with k + 96; an odd Kq cuts a pair and must keep the
    smaller id, in every tier. (The range tier needs more candidates than 3/4 of its smallest table,
    192: its queries take two such pairs, f = 1/4 -- still exact, every key still tied with its twin.)"""
    g, H = twin_graph()
    plan = ppr.GrankPlan(g, 8, 96, 0.85)  # L = the component size: no top-L cut inside a component
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    ids, sc, lens = slab
    for v in range(H):  # the premise: twin rows are identical up to the id shift
        n = int(lens[v])
        assert lens[v + H] == n
        assert np.array_equal(ids[v, :n] + H, ids[v + H, :n])
        assert np.array_equal(sc[v, :n].view(np.uint64), sc[v + H, :n].view(np.uint64))
    long_rows = [v for v in range(H) if lens[v] > 60]
    assert len(long_rows) >= 8
    if tier == "range":
        qs = [[a, a + H, b, b + H] for a, b in zip(long_rows[0:8:2], long_rows[1:8:2])]
        assert all(cand(lens, q) > 192 for q in qs)
    else:
        qs = [[v, v + H] for v in long_rows[:6] + [0, 7]]
    tot = [oracle_totals(slab, q, [1.0] * len(q)) for q in qs]
    for k, s in tot[0].items():
        assert tot[0][k + H if k < H else k - H] == s
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for Kq in (1, 7, 33):
        res = plan.query(qs, Kq, weights=[[1.0] * len(q) for q in qs])
        same_bits(res, oracle_rows(tot, qs, Kq))
        assert {"wave": res.wave_queries, "wg": res.wg_queries, "range": res.range_queries}[tier] == len(qs)
        cut = 0
        for q, t in enumerate(tot):  # the cut does fall inside a tie: the next key has the same score
            srt = sorted((-s, k) for k, s in t.items())
            if len(srt) > Kq:  # (the dangling pairs have two keys)
                assert srt[Kq - 1][0] == srt[Kq][0] and res.ids[q, Kq - 1] == srt[Kq - 1][1] < srt[Kq][1]
                cut += 1
        assert cut >= 4
    plan.close()


# ---- exclude_seeds, linearity, hot ids, slots, errors --------------------------------------------
def test_exclude_seeds(base, mixed):
    g, plan, slab = base
    for name in ("wave", "range"):
        qs, ws, tot = mixed[name]
        res = plan.query(qs, 16, weights=flat_weights(qs, ws), exclude_seeds=True)
        same_bits(res, oracle_rows(tot, qs, 16, exclude=True))
        for q, s in enumerate(qs):
            assert not set(res.ids[q, :res.lens[q]].tolist()) & set(s)
    assert res.range_queries > 0


def test_single_seed_linearity(base):
    """{v: 1.0} with Kq = L gives the slab row back: f = 1 and every score >= 2^-41, so
    floor(s * 2^93) is exact"""
    g, plan, slab = base
    ids, sc, lens = slab
    src = np.nonzero(lens > 1)[0][:50]
    assert len(src) == 50
    assert min(sc[v, :lens[v]].min() for v in src) >= 2.0 ** -41
    res = plan.query([[int(v)] for v in src], plan.L, weights=[[1.0]] * 50)
    assert np.array_equal(res.lens, lens[src])
    assert np.array_equal(res.ids, ids[src])
    assert np.array_equal(res.scores.view(np.uint64), sc[src].view(np.uint64))


def test_hot_encoded_ids(monkeypatch):
    """a chain-mode run with a forced hot set stores hot keys as tagged ids: queries decode them"""
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
    rng = np.random.default_rng(4)
    qs, ws = wave_queries(g.n, slab[2], rng)
    qs, ws = qs[:60] + [list(range(g.n))], ws[:60] + [None]
    res = plan.query(qs, 16, weights=flat_weights(qs, ws))
    same_bits(res, oracle_rows([oracle_totals(slab, q, w) for q, w in zip(qs, ws)], qs, 16))
    assert res.range_queries == 1
    plan.close()


def test_slot_selection_and_no_trace():
    g = ppr.rmat(10, seed=5)
    rng = np.random.default_rng(8)
    qs = [rng.integers(0, g.n, size=k).tolist() for k in (1, 5, 30, 200, 900)]
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.init()
    slab0 = plan.fetch_slab(0)
    res = plan.query(qs, 16, iterations_run=0)
    same_bits(res, oracle_rows([oracle_totals(slab0, q) for q in qs], qs, 16))
    plan.run(5, -1.0)  # an odd iteration count
    slab5 = plan.fetch_slab()
    res = plan.query(qs, 16)
    same_bits(res, oracle_rows([oracle_totals(slab5, q) for q in qs], qs, 16))
    assert not np.array_equal(slab0[1], slab5[1])
    # queries leave no trace: the plan runs again like a fresh one
    plan.run(6, -1.0)
    again = plan.fetch()
    fresh = ppr.GrankPlan(g, 16, 32, 0.85)
    fresh.run(6, -1.0)
    want = fresh.fetch()
    assert np.array_equal(again.ids, want.ids) and np.array_equal(again.scores, want.scores)
    assert np.array_equal(again.lens, want.lens)
    plan.close()
    fresh.close()


def test_errors_without_a_launch(base, monkeypatch):
    """every refusal is a host decision; the plan answers a normal query afterwards"""
    g, plan, slab = base
    lens = slab[2]

    def code(queries, K=16, weights=None, p=None):
        qptr, seeds, w = normalize_queries(queries, weights)
        Q = len(qptr) - 1
        ids = np.zeros((Q, max(K, 1)), dtype=np.int32)
        sc = np.zeros((Q, max(K, 1)))
        ln = np.zeros(Q, dtype=np.int32)
        return _lib.lib().ppr_grank_plan_query(p or plan._p, plan.iterations_run, Q, _lib.ptr(qptr), _lib.ptr(seeds),
                                               _lib.ptr(w), K, 0, _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(ln), None)

    assert code([[1, g.n]]) == 12                      # PPR_ERR_SOURCE
    assert code([[1, -1]]) == 12
    assert code([[1, 2]], weights=[[1.0, -1.0]]) == 1  # PPR_ERR_ARG
    assert code([[1, 2]], weights=[[1.0, float("nan")]]) == 1
    assert code([[1, 2]], weights=[[1.0, float("inf")]]) == 1
    assert code([[1, 2], []], weights=[[0.0, 0.0], []]) == 1
    assert code([[1]], K=0) == 2                       # PPR_ERR_K
    assert code([[1]], K=4097) == 11                   # PPR_ERR_RANGE
    ids = np.zeros(16, dtype=np.int32)
    qp = np.array([0, 1], dtype=np.int64)
    sd = np.array([1], dtype=np.int32)
    assert _lib.lib().ppr_grank_plan_query(plan._p, 6, 1, _lib.ptr(qp), _lib.ptr(sd), None, 16, 2, _lib.ptr(ids),
                                           _lib.ptr(np.zeros(16)), _lib.ptr(ids), None) == 1  # unknown flag bits
    mc = ppr.MccpPlan(g, 16, 32, 0.85)
    assert code([[1]], p=mc._p) == 1                   # an MC plan
    mc.close()
    # too wide: with 256-slot tables a key range takes 192 candidates; four times that per range on
    # average cannot fit whatever the distribution
    wide = list(range(g.n)) * 2
    assert cand(lens, wide) // 64 >= 4 * 192
    monkeypatch.setenv("PPR_Q_T", "256")
    assert code([[1, 2], wide]) == 11
    with pytest.raises(ppr.PprError):
        plan.query([wide], 16)
    monkeypatch.delenv("PPR_Q_T")
    qs = [[1, 2, 3], [10] * 3]
    res = plan.query(qs, 16)
    same_bits(res, oracle_rows([oracle_totals(slab, q) for q in qs], qs, 16))
