"""Reverse queries (GrankPlan.rquery / ppr_grank_plan_rquery) against their definition, restated with
Python integers from the plan's fetched slab: W summed in target order, f_j = w_j / W,
X_q[u] = sum over the targets t_j that are keys of B[u] of floor(fl(B[u][t_j] * f_j) * 2^93), score =
X * 2^-93 rounded once, the Kq best hit sources by (score desc, source id asc). Ids, score bits and
lens are compared exactly, through both tiers (scan, probe), every chunking, list batching, segment
size and query order."""
import math
from fractions import Fraction

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib
from approximated_personalized_pagerank_amd.grank import normalize_queries
from helpers import XSUM_RTOL

pytestmark = pytest.mark.gpu

XS_F = 93
# default knobs (csrc/rquery.hip): table slots, queries per chunk, probe-tier postings, list entries per batch
T_DEF, CHUNK_DEF, PROBE_DEF, ENTRIES_DEF = 8192, 4096, 16, 1 << 24


# ---- the oracle ---------------------------------------------------------------------------------
def column_index(slab):
    """{key: [(source, score)]}: the slab by columns, built once per slab"""
    ids, sc, lens = slab
    col = {}
    for u in range(len(lens)):
        for j in range(int(lens[u])):
            col.setdefault(int(ids[u, j]), []).append((u, float(sc[u, j])))
    return col


def xs_term(p):
    """floor(p * 2^93) of a double p >= 0, exactly"""
    num, den = p.as_integer_ratio()
    return (num << XS_F) // den


def oracle_scores(col, targets, weights=None):
    """{source: score} of one query by the definition (exact integers); every hit is a key"""
    ws = [1.0] * len(targets) if weights is None else [float(w) for w in weights]
    W = 0.0
    for w in ws:  # in target order
        W += w
    acc = {}
    for t, w in zip(targets, ws):
        f = w / W
        for u, s in col.get(int(t), ()):
            acc[u] = acc.get(u, 0) + xs_term(s * f)
    return {u: float(Fraction(x, 2 ** XS_F)) for u, x in acc.items()}


def oracle_rows(scores, targets_of, Kq, exclude=False):
    Q = len(scores)
    ids = np.full((Q, Kq), -1, dtype=np.int32)
    sc = np.zeros((Q, Kq), dtype=np.float64)
    lens = np.zeros(Q, dtype=np.int32)
    for q, t in enumerate(scores):
        drop = set(int(u) for u in targets_of[q]) if exclude else ()
        top = sorted(((-s, u) for u, s in t.items() if u not in drop))[:Kq]
        lens[q] = len(top)
        for i, (ms, u) in enumerate(top):
            ids[q, i] = u
            sc[q, i] = -ms
    return ids, sc, lens


def hit_counts(scores, targets_of, exclude=False):
    return [len(set(t) - set(int(u) for u in targets_of[q])) if exclude else len(t) for q, t in enumerate(scores)]


def same_bits(res, want):
    ids, sc, lens = want
    assert np.array_equal(res.lens, lens)
    assert np.array_equal(res.ids, ids)
    assert np.array_equal(res.scores.view(np.uint64), sc.view(np.uint64))


def expected_stats(qs, hits, n, Kq, T=T_DEF, chunk=CHUNK_DEF, probe_max=PROBE_DEF, entries=ENTRIES_DEF):
    """the host's rules restated (csrc/rquery.hip): chunks are runs of consecutive queries with at most
    3/4 T postings, `chunk` queries and 2^24 output entries; a chunk of 1 .. probe_max postings whose
    lists (n entries per non-empty query) fit E = max(entries, n) is probed; a scanned chunk with
    postings takes one count pass and one emit pass per batch of queries, in order, whose hits sum to
    at most E. Returns (chunks, probe_queries, scan_queries, scans)."""
    cap, E = 3 * T // 4, max(entries, n)
    chunks, cur, post = [], [], 0
    for i, q in enumerate(qs):
        if cur and (len(cur) >= chunk or post + len(q) > cap or (len(cur) + 1) * Kq > 1 << 24):
            chunks.append(cur)
            cur, post = [], 0
        cur.append(i)
        post += len(q)
    if cur:
        chunks.append(cur)
    pq = sq = scans = 0
    for c in chunks:
        post = sum(len(qs[i]) for i in c)
        nonempty = sum(len(qs[i]) > 0 for i in c)
        if 0 < post <= probe_max and nonempty * n <= E:
            pq += len(c)
            continue
        sq += len(c)
        if post == 0:
            continue
        batches, used = 1, 0
        for k, i in enumerate(c):
            if k and used + hits[i] > E:
                batches, used = batches + 1, 0
            used += hits[i]
        scans += 1 + batches
    return len(chunks), pq, sq, scans


def check_stats(res, qs, hits, n, Kq, **kw):
    assert res.hits == sum(hits)
    assert res.probe_queries + res.scan_queries == len(qs)
    assert (res.chunks, res.probe_queries, res.scan_queries, res.scans) == expected_stats(qs, hits, n, Kq, **kw)


def flat_weights(qs, ws):
    return np.concatenate([np.ones(len(q)) if w is None else np.asarray(w, dtype=np.float64)
                           for q, w in zip(qs, ws)] + [np.zeros(0)])


# ---- the base plan and the mixed query set -------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    g = ppr.rmat(10, seed=5)
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    col = column_index(slab)
    yield g, plan, slab, col
    plan.close()


def premises(col, n):
    """(the most frequent key, a rare key): the first sits in >= n / 2 rows, the second in <= 2"""
    freq = max(col, key=lambda k: (len(col[k]), -k))
    rare = min(col, key=lambda k: (len(col[k]), k))
    assert len(col[freq]) >= n // 2 and len(col[rare]) <= 2
    return freq, rare


def mixed_queries(n, freq, rare, rng):
    qs, ws = [[]], [None]                                          # an empty query
    qs.append([freq]); ws.append(None)                             # the most frequent target
    qs.append([rare]); ws.append(None)                             # a rare target
    qs.append([7, freq, 9, freq]); ws.append([1.0, 2.0, 0.5, 1.0])  # a repeated target, different weights
    qs.append([freq, 4, rare]); ws.append([0.0, 1.0, 0.0])         # zero weights: still hits, score 0
    while len(qs) < 305:
        k = int(rng.integers(0, 41))
        t = rng.integers(0, n, size=k).tolist()
        mode = len(qs) % 3
        ws.append(None if mode == 0 or k == 0 else
                  (rng.random(k) + 0.01).tolist() if mode == 1 else
                  rng.choice([0.0, 1.0, 2.0, 0.125], size=k).tolist())
        if ws[-1] is not None and sum(ws[-1]) == 0.0:
            ws[-1][0] = 1.0
        qs.append(t)
    for k in (300, 777):                                           # wide queries
        qs.append(rng.integers(0, n, size=k).tolist())
        ws.append((rng.random(k) + 0.1).tolist() if k == 777 else None)
    qs.append(list(range(n))); ws.append(None)                     # every node a target
    return qs, ws


@pytest.fixture(scope="module")
def mixed(base):
    g, plan, slab, col = base
    freq, rare = premises(col, g.n)
    qs, ws = mixed_queries(g.n, freq, rare, np.random.default_rng(11))
    return qs, ws, [oracle_scores(col, q, w) for q, w in zip(qs, ws)], freq, rare


def test_mixed_set_default_knobs(base, mixed):
    g, plan, slab, col = base
    qs, ws, tot, freq, rare = mixed
    n = g.n
    hits = hit_counts(tot, qs)
    assert hits[0] == 0 and hits[1] >= n // 2 and hits[2] <= 2 and hits[-1] == n
    assert hits[4] == len(set(u for k in (freq, 4, rare) for u, _ in col.get(k, ())))  # zero-weight targets hit
    for Kq in (1, 16, 200, n):
        res = plan.rquery(qs, Kq, weights=flat_weights(qs, ws))
        same_bits(res, oracle_rows(tot, qs, Kq))
        check_stats(res, qs, hits, n, Kq)
        assert res.chunks >= 2 and res.scans >= 4 and res.device_ms > 0 and res.algo_bytes > 0
    assert res.lens[0] == 0 and res.lens[2] <= 2 and res.lens[-1] == n  # Kq = n: whole columns, short rows
    zero = res.scores[4, :res.lens[4]] == 0.0
    assert zero.any() and not zero.all()
    # weights=None: every weight 1.0
    sub = [i for i, w in enumerate(ws) if w is None]
    res = plan.rquery([qs[i] for i in sub], 16)
    same_bits(res, oracle_rows([tot[i] for i in sub], [qs[i] for i in sub], 16))


def test_tier_and_batching_independence(base, mixed, monkeypatch):
    """the same queries through the other tier, other chunkings, list batchings, segment sizes, call
    splits and query orders: identical bits"""
    g, plan, slab, col = base
    qs0, ws0, tot0, freq, rare = mixed
    n = g.n
    pickq = list(range(5)) + list(range(5, 305, 4)) + [305, 306, 307]
    qs, ws, tot = [qs0[i] for i in pickq], [ws0[i] for i in pickq], [tot0[i] for i in pickq]
    qs += [[freq]] * 10                                            # ten lists of ~800 entries
    ws += [None] * 10
    tot += [tot0[1]] * 10
    Q, Kq = len(qs), 16
    want = oracle_rows(tot, qs, Kq)
    hits = hit_counts(tot, qs)

    def ask(idx, K=Kq):
        sub, wsub = [qs[i] for i in idx], [ws[i] for i in idx]
        return plan.rquery(sub, K, weights=flat_weights(sub, wsub))

    def rows(idx, w=want):
        return tuple(a[idx] for a in w)

    everything = list(range(Q))
    ref = ask(everything)
    same_bits(ref, want)
    check_stats(ref, qs, hits, n, Kq)

    with monkeypatch.context() as m:  # all scan
        m.setenv("PPR_R_PROBE_MAX", "0")
        res = ask(everything)
        same_bits(res, want)
        assert res.probe_queries == 0
        for i in (1, 2, 3):  # single-query calls too
            r1 = ask([i])
            same_bits(r1, rows([i]))
            assert (r1.probe_queries, r1.scan_queries) == (0, 1)

    with monkeypatch.context() as m:  # all probe: single-query calls
        m.setenv("PPR_R_PROBE_MAX", "100000")
        for i in everything[:40] + everything[-14:]:
            r1 = ask([i])
            same_bits(r1, rows([i]))
            assert (r1.probe_queries, r1.scan_queries, r1.scans) == ((1, 0, 0) if qs[i] else (0, 1, 0))
        r2 = ask([1, 2, 3])  # a chunk of three probed lists
        same_bits(r2, rows([1, 2, 3]))
        assert r2.probe_queries == 3

    with monkeypatch.context() as m:  # a 256-slot table: more chunks; more than 192 targets are refused
        m.setenv("PPR_R_T", "256")
        narrow = [i for i in everything if len(qs[i]) <= 192]
        assert 0 < Q - len(narrow) <= 3
        with pytest.raises(ppr.PprError) as e:
            ask(everything)  # a call that holds a refused query is refused whole
        assert e.value.code == 11
        res = ask(narrow)
        same_bits(res, rows(narrow))
        check_stats(res, [qs[i] for i in narrow], [hits[i] for i in narrow], n, Kq, T=256)
        assert res.chunks > ref.chunks

    with monkeypatch.context() as m:
        m.setenv("PPR_R_CHUNK", "7")
        res = ask(everything)
        same_bits(res, want)
        check_stats(res, qs, hits, n, Kq, chunk=7)
        assert res.chunks >= Q // 7

    with monkeypatch.context() as m:  # E falls to n: the ten ~800-entry lists need a batch each
        m.setenv("PPR_R_ENTRIES", "1")
        res = ask(everything)
        same_bits(res, want)
        check_stats(res, qs, hits, n, Kq, entries=1)
        assert res.scans >= ref.scans + 9

    with monkeypatch.context() as m:  # multi-level list reduction
        m.setenv("PPR_R_SEG", "64")
        assert max(hits) > 64 * 4
        for K in (16, 1, 50):
            res = ask(everything, K)
            same_bits(res, oracle_rows(tot, qs, K))
        m.setenv("PPR_R_PROBE_MAX", "100000")
        same_bits(ask([1]), rows([1]))

    for part in (everything[:Q // 2][::-1], everything[Q // 2:][::-1]):  # split calls, reversed order
        same_bits(ask(part), rows(part))


# ---- row shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,L", [(10, 100), (11, 200), (10, 30), (10, 70), (10, 300)])
def test_row_shapes(scale, L, monkeypatch):
    """L = 100 and 200 (rows narrower than the padded width; one 16-B load per lane with 32 and 64 lanes
    per row), L = 30 and 70 (not a multiple of 4: 4-B loads, one and two trips), L = 300 (rows longer
    than one 16-B load per lane). A probe-sized query, a mid one and a wide one whose rows overflow the
    per-wave table, each through both tiers."""
    g = ppr.rmat(scale, seed=5 + scale)
    plan = ppr.GrankPlan(g, 16, L, 0.85)
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    n = g.n
    # rows with more hits than the per-wave table (48) and, at L = 300, than a wave's hit buffer (256) take
    assert slab[2].max() > (256 if L == 300 else 48 if L > 48 else L - 1)
    col = column_index(slab)
    freq, rare = premises(col, n)
    rng = np.random.default_rng(scale * 1000 + L)
    qs = [[freq, rare, int(rng.integers(n))], rng.integers(0, n, size=20).tolist(), list(range(n))]
    ws = [None, (rng.random(20) + 0.1).tolist(), None]
    tot = [oracle_scores(col, q, w) for q, w in zip(qs, ws)]
    hits = hit_counts(tot, qs)
    for Kq in (50, n):
        want = oracle_rows(tot, qs, Kq)
        res = plan.rquery(qs, Kq, weights=flat_weights(qs, ws))
        same_bits(res, want)
        check_stats(res, qs, hits, n, Kq)
        assert res.scan_queries == 3
    small = plan.rquery(qs[:1], 50)
    same_bits(small, tuple(a[:1] for a in oracle_rows(tot, qs, 50)))
    assert (small.probe_queries, small.scans) == (1, 0)
    monkeypatch.setenv("PPR_R_PROBE_MAX", "100000")
    for i in (1, 2):
        r1 = plan.rquery([qs[i]], 50, weights=[ws[i]] if ws[i] else None)
        same_bits(r1, tuple(a[i:i + 1] for a in oracle_rows(tot, qs, 50)))
        assert r1.probe_queries == 1
    plan.close()


# ---- ties at the cut -----------------------------------------------------------------------------
def twin_graph():
    """two identical components of 96 nodes (ids v and v + 96), about 6 random successors per node,
    every seventh node dangling (the construction of test_gpu_query.py)"""
    rng = np.random.default_rng(3)
    H = 96
    succ = [[] if v % 7 == 0 else sorted(set(rng.integers(0, H, size=6).tolist())) for v in range(H)]
    rows = succ + [[s + H for s in r] for r in succ]
    rp = np.zeros(2 * H + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return ppr.Csr(rp, np.array([s for r in rows for s in r], dtype=np.int32)), H


def test_ties_at_the_cut(monkeypatch):
    """for a query {k, k + 96} with equal weights the sources v and v + 96 tie; an odd Kq cuts a pair and
    must keep the smaller id, in both tiers"""
    g, H = twin_graph()
    plan = ppr.GrankPlan(g, 8, 96, 0.85)
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    col = column_index(slab)
    keys = [k for k in range(H) if len(col.get(k, ())) > 40][:8]
    assert len(keys) >= 6
    qs = [[k, k + H] for k in keys]
    ws = [[1.0, 1.0]] * len(qs)
    tot = [oracle_scores(col, q, w) for q, w in zip(qs, ws)]
    for u, s in tot[0].items():  # the premise: twins tie
        assert tot[0][u + H if u < H else u - H] == s
    for tier in ("scan", "probe"):
        for Kq in (1, 7, 33):
            want = oracle_rows(tot, qs, Kq)
            if tier == "scan":
                with monkeypatch.context() as m:
                    m.setenv("PPR_R_PROBE_MAX", "0")
                    res = plan.rquery(qs, Kq, weights=ws)
                assert res.scan_queries == len(qs)
                got = (res.ids, res.scores, res.lens)
            else:
                rs = [plan.rquery([q], Kq, weights=[w]) for q, w in zip(qs, ws)]
                assert all(r.probe_queries == 1 for r in rs)
                got = tuple(np.concatenate([getattr(r, f) for r in rs]) for f in ("ids", "scores", "lens"))
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
            assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
            cut = 0
            for q, t in enumerate(tot):  # the cut does fall inside a tie: the next source has the same score
                srt = sorted((-s, u) for u, s in t.items())
                if len(srt) > Kq and srt[Kq - 1][0] == srt[Kq][0]:
                    assert got[0][q, Kq - 1] == srt[Kq - 1][1] < srt[Kq][1]
                    cut += 1
            assert cut >= 4
    plan.close()


# ---- exclusion, identities, hot ids, slots, errors -------------------------------------------------
def test_exclude_targets(base, mixed, monkeypatch):
    g, plan, slab, col = base
    qs0, ws0, tot0, freq, rare = mixed
    pickq = list(range(5)) + list(range(5, 305, 6)) + [305, 306, 307]
    qs, ws, tot = [qs0[i] for i in pickq], [ws0[i] for i in pickq], [tot0[i] for i in pickq]
    hub = next(u for u, _ in col[freq] if u != freq)                # a source that holds the frequent key
    qs += [[freq, hub], [hub]]                                     # targets that are hit sources
    ws += [None, None]
    tot += [oracle_scores(col, q) for q in qs[-2:]]
    assert hub in tot[-2]
    want = oracle_rows(tot, qs, 16, exclude=True)
    hits = hit_counts(tot, qs, exclude=True)
    assert sum(hits) < sum(hit_counts(tot, qs))
    res = plan.rquery(qs, 16, weights=flat_weights(qs, ws), exclude_targets=True)
    same_bits(res, want)
    check_stats(res, qs, hits, g.n, 16)
    assert res.scan_queries == len(qs)
    for q, t in enumerate(qs):
        assert not set(res.ids[q, :res.lens[q]].tolist()) & set(t)
    monkeypatch.setenv("PPR_R_PROBE_MAX", "100000")  # the probe tier
    for i in list(range(1, 12)) + [len(qs) - 4, len(qs) - 2, len(qs) - 1]:
        r1 = plan.rquery([qs[i]], 16, weights=None if ws[i] is None else [ws[i]], exclude_targets=True)
        same_bits(r1, tuple(a[i:i + 1] for a in want))
        assert r1.probe_queries == (1 if qs[i] else 0) and r1.hits == hits[i]


def test_column_identity(base, monkeypatch):
    """{t: 1.0} with Kq = n gives column t back: f = 1 and every score >= 2^-41, so floor(s * 2^93) is exact"""
    g, plan, slab, col = base
    ts = sorted(col, key=lambda k: (-len(col[k]), k))[:25] + sorted(col, key=lambda k: (len(col[k]), k))[:25]
    assert len(set(ts)) == 50 and min(s for t in ts for _, s in col[t]) >= 2.0 ** -41
    for env in ("0", "100000"):
        monkeypatch.setenv("PPR_R_PROBE_MAX", env)
        for lo in (0, 25):
            batch = ts[lo:lo + 25] if env == "0" else ts[lo:lo + 3]
            calls = [batch] if env == "0" else [[t] for t in batch]
            for call in calls:
                res = plan.rquery([[t] for t in call], g.n, weights=[[1.0]] * len(call))
                for q, t in enumerate(call):
                    k = int(res.lens[q])
                    assert k == len(col[t])
                    assert sorted(zip(res.ids[q, :k].tolist(), res.scores[q, :k].tolist())) == sorted(col[t])


def test_adjoint_identity_with_the_forward_query(base):
    """sum_{u in S} rquery_T(u) / |S| and sum_{t in T} query_S(t) / |T| are both
    sum B[u][t] / (|S| |T|), up to one floor of < 2^-93 and one rounding per term"""
    g, plan, slab, col = base
    rng = np.random.default_rng(21)
    n = g.n
    for ns, nt in [(1, 1), (5, 3), (40, 60), (300, 200)]:
        S = rng.choice(n, size=ns, replace=False).tolist()
        Tg = rng.choice(n, size=nt, replace=False).tolist()
        if ns <= 5:  # small sets that do meet: the targets come from the sources' own rows
            Tg = sorted(set(int(slab[0][S[i % ns], i % slab[2][S[i % ns]]]) for i in range(nt)))
            nt = len(Tg)
        rq = plan.rquery([Tg], n)
        fw = plan.query([S], n)
        # (nothing is cut: Kq = n)
        r = dict(zip(rq.ids[0, :rq.lens[0]].tolist(), rq.scores[0, :rq.lens[0]].tolist()))
        f = dict(zip(fw.ids[0, :fw.lens[0]].tolist(), fw.scores[0, :fw.lens[0]].tolist()))
        a = math.fsum(r.get(u, 0.0) for u in S) / ns
        b = math.fsum(f.get(t, 0.0) for t in Tg) / nt
        assert a > 0.0 and abs(a - b) <= XSUM_RTOL * max(a, b)


def test_hot_encoded_ids(monkeypatch):
    """a chain-mode run with a forced hot set stores hot keys as tagged ids: both tiers decode them"""
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
    col = column_index(slab)
    freq, rare = premises(col, g.n)
    qs, ws = mixed_queries(g.n, freq, rare, np.random.default_rng(4))
    qs, ws = qs[:60] + [list(range(g.n))], ws[:60] + [None]
    tot = [oracle_scores(col, q, w) for q, w in zip(qs, ws)]
    want = oracle_rows(tot, qs, 16)
    res = plan.rquery(qs, 16, weights=flat_weights(qs, ws))
    same_bits(res, want)
    assert res.scan_queries == len(qs)
    monkeypatch.setenv("PPR_R_PROBE_MAX", "100000")
    for i in list(range(1, 20)) + [len(qs) - 1]:
        r1 = plan.rquery([qs[i]], 16, weights=None if ws[i] is None else [ws[i]])
        same_bits(r1, tuple(a[i:i + 1] for a in want))
        assert r1.probe_queries == (1 if qs[i] else 0)
    plan.close()


def test_slot_selection_and_no_trace():
    g = ppr.rmat(10, seed=5)
    rng = np.random.default_rng(8)
    qs = [rng.integers(0, g.n, size=k).tolist() for k in (1, 3, 30, 200, 900)]
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.init()
    slab0 = plan.fetch_slab(0)
    col0 = column_index(slab0)
    for sub in (qs, qs[:1], qs[1:2]):  # scan, probe, probe
        res = plan.rquery(sub, 16, iterations_run=0)
        same_bits(res, oracle_rows([oracle_scores(col0, q) for q in sub], sub, 16))
    assert res.probe_queries == 1
    plan.run(5, -1.0)  # an odd iteration count
    slab5 = plan.fetch_slab()
    col5 = column_index(slab5)
    for sub in (qs, qs[:1], qs[1:2]):
        res = plan.rquery(sub, 16)
        same_bits(res, oracle_rows([oracle_scores(col5, q) for q in sub], sub, 16))
    assert not np.array_equal(slab0[1], slab5[1])
    # reverse queries leave no trace: the plan runs again like a fresh one
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
    g, plan, slab, col = base

    def code(queries, K=16, weights=None, p=None, flags=0):
        qptr, targets, w = normalize_queries(queries, weights)
        Q = len(qptr) - 1
        ids = np.zeros((Q, max(K, 1)), dtype=np.int32)
        sc = np.zeros((Q, max(K, 1)))
        ln = np.zeros(Q, dtype=np.int32)
        return _lib.lib().ppr_grank_plan_rquery(p or plan._p, plan.iterations_run, Q, _lib.ptr(qptr), _lib.ptr(targets),
                                                _lib.ptr(w), K, flags, _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(ln), None)

    assert code([[1, g.n]]) == 12                      # PPR_ERR_SOURCE
    assert code([[1, -1]]) == 12
    assert code([[1, 2]], weights=[[1.0, -1.0]]) == 1  # PPR_ERR_ARG
    assert code([[1, 2]], weights=[[1.0, float("nan")]]) == 1
    assert code([[1, 2]], weights=[[1.0, float("inf")]]) == 1
    assert code([[1, 2], []], weights=[[0.0, 0.0], []]) == 1
    assert code([[1, 2]], weights=[[1e308, 1e308]]) == 1  # W not finite
    assert code([[1]], flags=2) == 1                   # unknown flag bits
    assert code([[1]], K=0) == 2                       # PPR_ERR_K
    assert code([[1]], K=4097) == 11                   # PPR_ERR_RANGE
    assert code([[1], [5] * 6145]) == 11               # more targets than 3/4 of the 8192-slot table
    assert code([[5] * 6144], K=1) == 0
    qp = np.array([0, 2, 1], dtype=np.int64)           # non-monotone qptr
    sd = np.array([1, 2], dtype=np.int32)
    ids = np.zeros(32, dtype=np.int32)
    assert _lib.lib().ppr_grank_plan_rquery(plan._p, 6, 2, _lib.ptr(qp), _lib.ptr(sd), None, 16, 0, _lib.ptr(ids),
                                            _lib.ptr(np.zeros(32)), _lib.ptr(ids), None) == 1
    qp = np.array([0, 1], dtype=np.int64)
    assert _lib.lib().ppr_grank_plan_rquery(plan._p, 6, 1, _lib.ptr(qp), _lib.ptr(sd), None, 16, 0, None, None, None,
                                            None) == 1  # null outputs
    assert _lib.lib().ppr_grank_plan_rquery(plan._p, 6, -1, _lib.ptr(qp), _lib.ptr(sd), None, 16, 0, _lib.ptr(ids),
                                            _lib.ptr(np.zeros(32)), _lib.ptr(ids), None) == 1  # Q < 0
    mc = ppr.MccpPlan(g, 16, 32, 0.85)
    assert code([[1]], p=mc._p) == 1                   # an MC plan
    mc.close()
    monkeypatch.setenv("PPR_R_T", "256")
    assert code([[1, 2], [3] * 193]) == 11
    with pytest.raises(ppr.PprError):
        plan.rquery([[3] * 193], 16)
    monkeypatch.delenv("PPR_R_T")
    qs = [[1, 2, 3], [10] * 3]
    res = plan.rquery(qs, 16)
    same_bits(res, oracle_rows([oracle_scores(col, q) for q in qs], qs, 16))
