"""PPR-induced subgraph batches from a plan's resident baskets (GrankPlan.subgraphs; include/ppr_hip.h
ppr_grank_plan_subgraphs) against the definition restated in Python from the fetched slab and the CSR:
the members of a position are its row ordered by (score desc, key asc), the root moved to the front
on request, cut at `size`; the edges are the stored edges between members, in (rank of the emitter,
position in the edge array) order. Every array is compared as integers, the scores as bit patterns."""
import ctypes

import numpy as np
import pytest
import torch

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

import graphs
import test_gpu_sweep as sweep_tests  # (its graph families and ring_of_cliques)

pytestmark = pytest.mark.gpu

ARG, RANGE, SOURCE = 1, 11, 12


# ---- the definition -----------------------------------------------------------------------------
def members(ids, sc, ln, u, size, root_first):
    ks = [k for _, k in sorted((-float(sc[u, j]), int(ids[u, j])) for j in range(ln[u]))]
    if root_first and u in ks:
        ks.remove(u); ks.insert(0, u)
    return ks[:size]


def induced(rp, col, ms, max_deg):
    rank = {k: j for j, k in enumerate(ms)}
    out = []                       # (rank a, rank b, p), already in contract order
    for j, k in enumerate(ms):
        if max_deg and rp[k + 1] - rp[k] > max_deg:
            continue
        for p in range(rp[k], rp[k + 1]):
            b = rank.get(int(col[p]) & 0x7fffffff)
            if b is not None:
                out.append((j, b, p))
    return out


def induced_np(rp, col, ms, max_deg, n):
    """induced() with the inner loop in numpy: an [E, 3] array (test_definition holds the two against each other)"""
    rank = np.full(n, -1, dtype=np.int64)
    rank[ms] = np.arange(len(ms))
    out = [np.zeros((0, 3), dtype=np.int64)]
    for j, k in enumerate(ms):
        if max_deg and rp[k + 1] - rp[k] > max_deg:
            continue
        b = rank[col[rp[k]:rp[k + 1]] & 0x7fffffff]
        hit = np.flatnonzero(b >= 0)
        out.append(np.stack([np.full(len(hit), j, dtype=np.int64), b[hit], int(rp[k]) + hit], axis=1))
    return np.concatenate(out)


class Oracle:
    """the expected batch of a list of sources; a source's own rows are computed once per argument set"""

    def __init__(self, g, slab):
        self.g, self.slab, self.cache = g, slab, {}

    def one(self, u, size, root_first, max_deg):
        key = (u, size, root_first, max_deg)
        if key not in self.cache:
            ids, sc, ln = self.slab
            rp, col = self.g.row_ptr, self.g.col
            ms = members(ids, sc, ln, u, size, root_first)
            ed = induced_np(rp, col, ms, max_deg, self.g.n)
            row_sc = {int(ids[u, j]): sc[u, j] for j in range(ln[u])}
            deg = [int(rp[k + 1] - rp[k]) for k in ms]
            capped = sum(1 for d in deg if max_deg and d > max_deg)
            walked = sum(d for d in deg if not (max_deg and d > max_deg))
            self.cache[key] = (ms, np.array([row_sc[k] for k in ms], dtype=np.float64), ed, walked, capped)
        return self.cache[key]

    def batch(self, sources, size=None, root_first=False, max_deg=0):
        nodes, scs, rowptr, colb, rowb, eid, node_ptr, edge_ptr = [], [], [], [], [], [], [0], [0]
        walked = capped = 0
        for u in sources:
            ms, s, ed, w, c = self.one(int(u), size, root_first, max_deg)
            n0, e0 = node_ptr[-1], edge_ptr[-1]
            per = np.bincount(ed[:, 0], minlength=len(ms))
            rowptr += (e0 + np.concatenate(([0], np.cumsum(per)[:-1]))).tolist() if ms else []
            nodes += ms
            scs.append(s)
            rowb.append(n0 + ed[:, 0])
            colb.append(n0 + ed[:, 1])
            eid.append(ed[:, 2])
            node_ptr.append(n0 + len(ms))
            edge_ptr.append(e0 + len(ed))
            walked += w
            capped += c
        rowptr.append(edge_ptr[-1])
        i64 = lambda x: np.asarray(x, dtype=np.int64)
        cat = lambda x: np.concatenate(x) if x else np.zeros(0, dtype=np.int64)
        return dict(nodes=i64(nodes), scores=np.concatenate(scs) if scs else np.zeros(0), rowptr=i64(rowptr), col=cat(colb),
                    row=cat(rowb), eid=cat(eid), node_ptr=i64(node_ptr), edge_ptr=i64(edge_ptr), walked=walked, capped=capped)


def host(t):
    return None if t is None else t.cpu().numpy()


def check(b, want, index_dtype=torch.int64, st=None):
    assert np.array_equal(b.node_ptr, want["node_ptr"]) and np.array_equal(b.edge_ptr, want["edge_ptr"])
    for f in ("nodes", "rowptr", "col", "row"):
        t = getattr(b, f)
        assert t.dtype == index_dtype and t.is_cuda, f
        assert np.array_equal(host(t).astype(np.int64), want[f]), f
    assert b.eid.dtype == torch.int64 and np.array_equal(host(b.eid), want["eid"])
    assert b.scores.dtype == torch.float64
    assert np.array_equal(host(b.scores).view(np.uint64), want["scores"].view(np.uint64))
    if st is not None:
        assert (st["nodes"], st["edges"], st["edges_walked"], st["capped_members"]) == \
            (len(want["nodes"]), len(want["col"]), want["walked"], want["capped"])


def same(a, b):
    assert np.array_equal(a.node_ptr, b.node_ptr) and np.array_equal(a.edge_ptr, b.edge_ptr)
    for f in ("nodes", "rowptr", "col", "row", "eid"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), f
    assert torch.equal(a.scores.view(torch.int64), b.scores.view(torch.int64))


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
        _plans[name] = (g, plan, slab, Oracle(g, slab))
    return _plans[name]


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for _, plan, _, _ in _plans.values():
        plan.close()
    _plans.clear()


# ---- 1. the definition --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_definition(name):
    g, plan, slab, orc = plan_of(name)
    rng = np.random.default_rng(11)
    some = [int(u) for u in rng.integers(0, g.n, size=40)]
    some += some[:5] + [some[0]] * 3 + [0, g.n - 1]
    if name == "sparse600":  # rows of length 1: a one-node subgraph whose only possible edge is a self-loop
        lens = slab[2]
        assert (lens == 1).sum() > 0
        some += [int(u) for u in np.flatnonzero(lens == 1)[:4]]
    for u in some[:6]:  # the oracle's numpy loop is the definition's loop
        for size, rf, md in ((None, False, 0), (20, True, 0), (None, True, 5)):
            ms = members(*slab, u, size, rf)
            assert induced_np(g.row_ptr, g.col, ms, md, g.n).tolist() == [list(e) for e in induced(g.row_ptr, g.col, ms, md)]
    for sources, src_arg in ((list(range(g.n)), None), (some, some)):
        for size in (None, 20, 1):
            want = orc.batch(sources, size)
            for dt in (torch.int32, torch.int64):
                st = {}
                b = plan.subgraphs(src_arg, size=size, index_dtype=dt, coo=True, edge_ids=True, scores=True, stats=st)
                check(b, want, dt, st)
                assert st["wave_sources"] + st["wg_sources"] + st["slice_sources"] == len(sources)
                N, E = b.num_nodes, b.num_edges
                rp = b.rowptr.to(torch.int64)
                assert torch.equal(b.row.to(torch.int64), torch.repeat_interleave(torch.arange(N, device=rp.device), rp[1:] - rp[:-1]))
                m = torch.sparse_csr_tensor(b.rowptr, b.col, torch.ones(E, device=rp.device), size=(N, N))
                assert m.shape == (N, N) and m.values().numel() == E
                if size == 1:  # one member each: only its self-loops
                    assert N == len(sources) and torch.equal(b.col, b.row)
                    assert np.array_equal(host(b.nodes)[host(b.col)], (g.col[host(b.eid)] & 0x7fffffff))
    if name == "sparse600":
        ones = [int(u) for u in np.flatnonzero(slab[2] == 1)]
        b = plan.subgraphs(ones, edge_ids=True)
        assert b.num_nodes == len(ones) and host(b.nodes).tolist() == ones  # (a row of length 1 holds its own source)
        loops = sum(int((g.col[g.row_ptr[u]:g.row_ptr[u + 1]] == u).sum()) for u in ones)
        assert b.num_edges == loops


# ---- 2. the tiers, the slices, the chunks, the order of the sources -----------------------------
def test_tier_independence(monkeypatch):
    g, plan, slab, orc = plan_of("multi500")
    ids, sc, lens = slab
    sources = list(range(g.n))
    want = orc.batch(sources, None, root_first=True)
    # the preconditions of this input
    assert np.all(lens == 32)
    per = np.diff(want["edge_ptr"])
    assert (int(per.min()), int(per.max()), int(per.sum())) == (89, 3306, 132080)
    deg = np.diff(g.row_ptr)
    W = [sum(int(deg[k]) for k in orc.one(u, None, True, 0)[0]) for u in sources]
    assert max(W) == 6617
    assert deg[0] == 3003 and any(0 in orc.one(u, None, True, 0)[0] for u in sources)
    st = {}
    base = plan.subgraphs(root_first=True, edge_ids=True, stats=st)
    check(base, want, torch.int64, st)
    assert st["chunks"] == 1
    big = 1 << 30
    forced = {"wave": dict(PPR_SG_WAVE_MAX=big), "wg": dict(PPR_SG_WAVE_MAX=0, PPR_SG_WG_MAX=big),
              "slice": dict(PPR_SG_WAVE_MAX=0, PPR_SG_WG_MAX=0, PPR_SG_SLICE=1024)}
    for tier, env in forced.items():
        for extra in ({}, dict(PPR_SG_CHUNK=7)):
            with monkeypatch.context() as mp:
                for k, v in {**env, **extra}.items():
                    mp.setenv(k, str(v))
                st = {}
                res = plan.subgraphs(root_first=True, edge_ids=True, stats=st)
                same(res, base)
                assert st[tier + "_sources"] == g.n and st["edges"] == 132080 and st["edges_walked"] == sum(W)
                assert st["chunks"] == ((g.n + 6) // 7 if extra else 1)
                rev = plan.subgraphs(sources[::-1], root_first=True, edge_ids=True, stats=st)
                assert st[tier + "_sources"] == g.n
            # reversed sources: every position has the same rows up to its offsets
            check(rev, orc.batch(sources[::-1], None, root_first=True))
            rn, re_ = rev.node_ptr, rev.edge_ptr
            bn, be = base.node_ptr, base.edge_ptr
            rv = {f: host(getattr(rev, f)) for f in ("nodes", "scores", "rowptr", "col", "row", "eid")}
            bs = {f: host(getattr(base, f)) for f in ("nodes", "scores", "rowptr", "col", "row", "eid")}
            for i in (0, 1, 250, 498, 499):
                j = g.n - 1 - i
                assert np.array_equal(rv["nodes"][rn[j]:rn[j + 1]], bs["nodes"][bn[i]:bn[i + 1]])
                assert np.array_equal(rv["scores"][rn[j]:rn[j + 1]].view(np.uint64), bs["scores"][bn[i]:bn[i + 1]].view(np.uint64))
                assert np.array_equal(rv["rowptr"][rn[j]:rn[j + 1]] - re_[j], bs["rowptr"][bn[i]:bn[i + 1]] - be[i])
                for f in ("col", "row"):
                    assert np.array_equal(rv[f][re_[j]:re_[j + 1]] - rn[j], bs[f][be[i]:be[i + 1]] - bn[i]), f
                assert np.array_equal(rv["eid"][re_[j]:re_[j + 1]], bs["eid"][be[i]:be[i + 1]])


# ---- 3. ties at the member cut ------------------------------------------------------------------
def test_ties_at_the_cut():
    g, plan, slab, orc = plan_of("layered16")
    ids, sc, lens = slab
    for size, rows_with_tie in ((20, 64), (17, 32)):
        tied = 0
        for u in range(g.n):
            s = np.sort(sc[u, :lens[u]])[::-1]
            assert lens[u] > size
            tied += int(s[size - 1] == s[size])  # the last member kept and the first one dropped score the same
        assert tied == rows_with_tie
        b = plan.subgraphs(size=size, edge_ids=True)
        check(b, orc.batch(range(g.n), size))
        # the smaller key wins: among the keys that tie with the last member, the kept ones are the smallest
        nodes = host(b.nodes)
        for u in range(g.n):
            kept = set(nodes[b.node_ptr[u]:b.node_ptr[u + 1]].tolist())
            row = {int(k): float(v) for k, v in zip(ids[u, :lens[u]], sc[u, :lens[u]])}
            cut = min(row[k] for k in kept)
            tie = sorted(k for k, v in row.items() if v == cut)
            inside = [k for k in tie if k in kept]
            assert inside == tie[:len(inside)]


# ---- 4. the root first --------------------------------------------------------------------------
def test_root_first():
    lists = []
    for i in range(40):
        lists += [[2 * i + 1], [2 * i + 1, (2 * i + 2) % 80]]
    g = ppr.Csr(*graphs._csr(lists))
    plan = ppr.GrankPlan(g, 8, 8, 0.85)
    plan.run(12, -1.0)
    slab = plan.fetch_slab()
    ids, sc, lens = slab
    orc = Oracle(g, slab)
    tops = [members(ids, sc, lens, u, 1, False)[0] for u in range(g.n)]
    assert sum(1 for u in range(g.n) if tops[u] != u) == 40
    plain = plan.subgraphs(edge_ids=True)
    first = plan.subgraphs(root_first=True, edge_ids=True)
    check(plain, orc.batch(range(g.n)))
    check(first, orc.batch(range(g.n), root_first=True))
    assert host(plain.nodes)[plain.node_ptr[:-1]].tolist() == tops
    assert host(first.nodes)[first.node_ptr[:-1]].tolist() == list(range(g.n))
    assert torch.equal(first.nodes[first.roots], torch.arange(g.n, device=first.nodes.device))
    # self-loops are edges of the subgraph
    assert int((first.row == first.col).sum()) > 0
    for size in (1, 3):
        check(plan.subgraphs(size=size, root_first=True, edge_ids=True), orc.batch(range(g.n), size, root_first=True))
    plan.close()


# ---- 5. it samples what it should ---------------------------------------------------------------
def test_samples_the_clique():
    g = sweep_tests.ring_of_cliques()
    plan = ppr.GrankPlan(g, 16, 64, 0.85)
    plan.run(20, -1.0)
    b = plan.subgraphs(size=16, edge_ids=True)
    check(b, Oracle(g, plan.fetch_slab()).batch(range(g.n), 16))
    nodes, col, row = host(b.nodes), host(b.col), host(b.row)
    assert g.n == 128 and np.all(np.diff(b.node_ptr) == 16) and np.all(np.diff(b.edge_ptr) == 240)
    for u in range(g.n):
        mine = nodes[b.node_ptr[u]:b.node_ptr[u + 1]]
        assert sorted(mine.tolist()) == list(range(u // 16 * 16, u // 16 * 16 + 16)) and mine[0] == u
    assert np.all(nodes[col] // 16 == nodes[row] // 16)  # no bridge edge
    assert torch.equal(b.batch, torch.arange(128, device=b.nodes.device).repeat_interleave(16))
    plan.close()


# ---- 6. max_deg ---------------------------------------------------------------------------------
def test_max_deg():
    g, plan, slab, orc = plan_of("multi500")
    want = orc.batch(range(g.n), max_deg=100)
    st = {}
    b = plan.subgraphs(max_deg=100, edge_ids=True, stats=st)
    check(b, want, torch.int64, st)
    assert st["capped_members"] == want["capped"] > 0 and st["edges_walked"] == want["walked"]
    assert st["edges_walked"] < orc.batch(range(g.n))["walked"]
    nodes, col, row = host(b.nodes), host(b.col), host(b.row)
    assert (nodes == 0).sum() > 0 and not np.any(nodes[row] == 0) and np.any(nodes[col] == 0)


# ---- 7. the capacity protocol -------------------------------------------------------------------
SENT = -77


def raw_call(plan, sources="all", S=None, size=0, max_deg=0, flags=0, node_cap=None, edge_cap=None, alloc=(64, 64), p=None,
             it=None, nulls=(), count_only=False):
    """the C call on sentinel-filled host and device outputs; returns (code, host arrays, device tensors)"""
    n = plan.csr.n
    src = None if isinstance(sources, str) else np.ascontiguousarray(sources, dtype=np.int32)
    if src is not None and len(src) == 0:
        src = np.zeros(1, dtype=np.int32)
    R = (n if isinstance(sources, str) else len(sources)) if S is None else S
    hostp = dict(node_ptr=np.full(max(R, 0) + 1, SENT, np.int64), edge_ptr=np.full(max(R, 0) + 1, SENT, np.int64))
    dt = torch.int64 if flags & 2 else torch.int32
    dev = torch.device("cuda", plan.device)
    na, ea = alloc
    t = dict(nodes=torch.full((na,), SENT, dtype=dt, device=dev), scores=torch.full((na,), float(SENT), dtype=torch.float64, device=dev),
             rowptr=torch.full((na + 1,), SENT, dtype=dt, device=dev), col=torch.full((ea,), SENT, dtype=dt, device=dev),
             row=torch.full((ea,), SENT, dtype=dt, device=dev), eid=torch.full((ea,), SENT, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    ptr = {k: (None if (k in nulls or count_only) else v.data_ptr()) for k, v in t.items()}
    hp = {k: (None if k in nulls else _lib.ptr(v)) for k, v in hostp.items()}
    rc = _lib.lib().ppr_grank_plan_subgraphs(
        plan._p if p is None else p, plan.iterations_run if it is None else it, R, _lib.ptr(src), size, max_deg, flags,
        (0 if count_only else na) if node_cap is None else node_cap, (0 if count_only else ea) if edge_cap is None else edge_cap,
        hp["node_ptr"], hp["edge_ptr"], ptr["nodes"], ptr["scores"], ptr["rowptr"], ptr["col"], ptr["row"], ptr["eid"], None)
    return rc, hostp, t


def untouched(hostp, t):
    return all(np.all(v == SENT) for v in hostp.values()) and all(bool((v == SENT).all()) for v in t.values())


def test_capacity_protocol(monkeypatch):
    g, plan, slab, orc = plan_of("rmat10")
    rng = np.random.default_rng(3)
    src = [int(u) for u in rng.integers(0, g.n, size=60)]
    want = orc.batch(src, 20)
    N, E = len(want["nodes"]), len(want["col"])
    assert N > 64 and E > 64
    full = plan.subgraphs(src, size=20, index_dtype=torch.int32, edge_ids=True)
    check(full, want, torch.int32)
    # count-only: the host arrays of the full call
    rc, hp, t = raw_call(plan, src, size=20, count_only=True)
    assert rc == 0 and np.array_equal(hp["node_ptr"], want["node_ptr"]) and np.array_equal(hp["edge_ptr"], want["edge_ptr"])
    assert all(bool((v == SENT).all()) for v in t.values())
    # exact capacities in longer tensors: the tails stay as they were
    rc, hp, t = raw_call(plan, src, size=20, node_cap=N, edge_cap=E, alloc=(N + 64, E + 64))
    assert rc == 0
    for f, k in (("nodes", N), ("rowptr", N + 1), ("col", E), ("row", E), ("eid", E)):
        assert np.array_equal(host(t[f][:k]).astype(np.int64), want[f]), f
        assert bool((t[f][k:] == SENT).all()), f
    assert np.array_equal(host(t["scores"][:N]).view(np.uint64), want["scores"].view(np.uint64)) and bool((t["scores"][N:] == SENT).all())
    # one edge / one node short: PPR_ERR_RANGE, the host arrays complete, nothing at or beyond the capacity
    for ncap, ecap in ((N, E - 1), (N - 1, E), (N - 1, E - 1), (N, 0), (0, E)):
        rc, hp, t = raw_call(plan, src, size=20, node_cap=ncap, edge_cap=ecap, alloc=(N + 64, E + 64))
        assert rc == RANGE, (ncap, ecap)
        assert np.array_equal(hp["node_ptr"], want["node_ptr"]) and np.array_equal(hp["edge_ptr"], want["edge_ptr"])
        for f in ("nodes", "scores", "rowptr"):
            assert bool((t[f][ncap:] == SENT).all()) or (f == "rowptr" and ncap == N and bool((t[f][N + 1:] == SENT).all())), f
        for f in ("col", "row", "eid"):
            assert bool((t[f][ecap:] == SENT).all()), f
    # the Python surface: a capacity that is too small costs one more call, an ample one none
    for cap in (E, E + 1000, E - 1, 0):
        check(plan.subgraphs(src, size=20, index_dtype=torch.int32, edge_ids=True, edge_capacity=cap), want, torch.int32)
    # several chunks with a capacity that runs out in the middle
    with monkeypatch.context() as mp:
        mp.setenv("PPR_SG_CHUNK", "7")
        rc, hp, t = raw_call(plan, src, size=20, node_cap=N, edge_cap=E // 2, alloc=(N + 64, E + 64))
    assert rc == RANGE and np.array_equal(hp["edge_ptr"], want["edge_ptr"]) and bool((t["col"][E // 2:] == SENT).all())


# ---- 8. hot-encoded ids and the slot rule -------------------------------------------------------
def test_hot_encoded_ids_and_slot_rule(monkeypatch):
    g = ppr.rmat(10, seed=5)
    with monkeypatch.context() as mp:
        for k, v in {"PPR_HOT_N": "64", "PPR_HOT_AT": "1", "PPR_TIER_MASK": "0x20"}.items():
            mp.setenv(k, v)
        plan = ppr.GrankPlan(g, 16, 32, 0.85, sum_mode="chain")
        plan.run(6, -1.0)
        raw = np.zeros((g.n, 32), dtype=np.int32)
        rl = np.zeros(g.n, dtype=np.int32)
        hot = 0
        for slot in (0, 1):
            _lib.check(_lib.lib().ppr_plan_fetch_slot(plan._p, slot, _lib.ptr(raw), None, _lib.ptr(rl)))
            hot += sum(int((raw[v, :rl[v]] < 0).sum()) for v in range(g.n))
        assert hot > 0  # the slab does hold tagged ids
        src = [int(u) for u in np.random.default_rng(8).integers(0, g.n, size=150)]
        check(plan.subgraphs(src, root_first=True, edge_ids=True), Oracle(g, plan.fetch_slab()).batch(src, root_first=True))
        plan.close()
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    src = [int(u) for u in np.random.default_rng(9).integers(0, g.n, size=100)]
    for it in (1, 2, 3):
        plan.run(it, -1.0)
        check(plan.subgraphs(src, size=12, edge_ids=True), Oracle(g, plan.fetch_slab()).batch(src, 12))
    check(plan.subgraphs(src, size=12, edge_ids=True, iterations_run=2), Oracle(g, plan.fetch_slab(2)).batch(src, 12))
    plan.close()


# ---- 9. edges of the contract -------------------------------------------------------------------
def test_contract_edges():
    g, plan, slab, orc = plan_of("sparse600")
    before = plan.fetch()
    for dt in (torch.int32, torch.int64):
        e = plan.subgraphs([], index_dtype=dt, edge_ids=True)  # an empty list is not "all"
        assert e.num_graphs == 0 and e.num_nodes == 0 and e.num_edges == 0
        assert e.nodes.shape == (0,) and e.col.shape == (0,) and e.rowptr.tolist() == [0] and e.edge_index.shape == (2, 0)
        assert e.node_ptr.tolist() == [0] and e.edge_ptr.tolist() == [0]
    rc, hp, t = raw_call(plan, [], S=0)
    assert rc == 0 and hp["node_ptr"].tolist() == [0] and hp["edge_ptr"].tolist() == [0] and int(t["rowptr"][0]) == 0
    # size above the row length: the whole row
    src = list(range(0, g.n, 7))
    check(plan.subgraphs(src, size=4096, edge_ids=True), orc.batch(src, 4096))
    same(plan.subgraphs(src, size=4096, edge_ids=True), plan.subgraphs(src, edge_ids=True))
    # the optional outputs off
    b = plan.subgraphs(src, coo=False, scores=False)
    assert b.row is None and b.eid is None and b.scores is None
    assert np.array_equal(host(b.col), orc.batch(src)["col"])
    # nothing was written into the plan
    after = plan.fetch()
    assert np.array_equal(before.ids, after.ids) and np.array_equal(before.scores.view(np.uint64), after.scores.view(np.uint64))
    assert all(np.array_equal(a, c) for a, c in zip(slab, plan.fetch_slab()))
    _, K, L, it = GRAPHS["sparse600"]
    plan.run(it, -1.0)
    assert all(np.array_equal(a, c) for a, c in zip(slab, plan.fetch_slab()))


# ---- 10. refusals -------------------------------------------------------------------------------
def test_refusals():
    g, plan, slab, orc = plan_of("rmat10")
    n = g.n
    some = [1, 2, 3]
    cases = [
        (ARG, dict(sources=some, p=0)),                              # a null plan
        (ARG, dict(sources=some, it=-1)),
        (ARG, dict(sources=some, nulls=("node_ptr",))),
        (ARG, dict(sources=some, nulls=("edge_ptr",))),
        (ARG, dict(sources=some, S=-1)),
        (ARG, dict(sources="all", S=n - 1)),                         # NULL sources with S != n
        (ARG, dict(sources=some, flags=4)),
        (ARG, dict(sources=some, flags=1 << 31)),
        (ARG, dict(sources=some, max_deg=-1)),
        (ARG, dict(sources=some, node_cap=-1)),
        (ARG, dict(sources=some, edge_cap=-1)),
        (ARG, dict(sources=some, nulls=("nodes",))),                 # some but not all required device pointers
        (ARG, dict(sources=some, nulls=("rowptr",))),
        (ARG, dict(sources=some, nulls=("col",))),
        (ARG, dict(sources=some, nulls=("nodes", "rowptr"))),
        (ARG, dict(sources=some, nulls=("nodes", "rowptr", "col"))),              # count-only with optional pointers
        (ARG, dict(sources=some, nulls=("nodes", "rowptr", "col", "scores", "row", "eid"))),  # ... with capacities
        (RANGE, dict(sources=some, size=4097)),
        (SOURCE, dict(sources=[1, n, 2])),
        (SOURCE, dict(sources=[-1])),
        # the order when two apply
        (ARG, dict(sources=some, size=4097, flags=8)),               # flags before the range
        (ARG, dict(sources=some, size=4097, max_deg=-3)),
        (ARG, dict(sources=some, size=4097, nulls=("col",))),
        (ARG, dict(sources=[n], S=-1)),                              # S before the sources
        (ARG, dict(sources=[n], max_deg=-1)),
        (RANGE, dict(sources=[n], size=4097)),                       # the range before the sources
        (ARG, dict(sources="all", S=n + 1, size=4097)),
    ]
    for want, kw in cases:
        rc, hp, t = raw_call(plan, **kw)
        assert rc == want, kw
        assert untouched(hp, t), kw
    # S > 2^30 is decided before a source is read (the pointer is never followed)
    L = _lib.lib()
    one = np.zeros(1, dtype=np.int32)
    hp = np.full(2, SENT, np.int64)
    assert L.ppr_grank_plan_subgraphs(plan._p, plan.iterations_run, (1 << 30) + 1, _lib.ptr(one), 0, 0, 0, 0, 0, _lib.ptr(hp),
                                      _lib.ptr(hp), None, None, None, None, None, None, None) == RANGE
    assert np.all(hp == SENT)
    # an MC plan
    mc = ppr.MccpPlan(g, 16, 64, 0.85)
    rc, hp, t = raw_call(plan, sources=some, p=mc._p)
    assert rc == ARG and untouched(hp, t)
    mc.close()
    # the stats are cleared by a refused call
    st = _lib.PprSubgStats()
    st.edges = 9
    assert L.ppr_grank_plan_subgraphs(plan._p, plan.iterations_run, -1, None, 0, 0, 0, 0, 0, None, None, None, None, None, None,
                                      None, None, ctypes.byref(st)) == ARG and st.edges == 0
    # the Python surface raises with the code
    with pytest.raises(ppr.PprError) as e:
        plan.subgraphs(some, size=5000)
    assert e.value.code == RANGE
    with pytest.raises(ppr.PprError) as e:
        plan.subgraphs([n])
    assert e.value.code == SOURCE
    with pytest.raises(TypeError):
        plan.subgraphs(some, index_dtype=torch.int16)
