"""Sweep-cut local clustering from a plan's resident baskets (GrankPlan.sweep / sweep_vectors;
include/ppr_hip.h) against its definition restated in Python integers from the fetched slab and the
CSR: r = s / max(deg, 1) in one fp64 divide, the order (r desc, key asc), the max_size and volume
stops, the integer profile of every prefix, the exact argmin of cut / den with ties to the smaller
prefix. order, swept, size, cut, vol and the profiles are compared as integers, phi as a bit pattern."""
import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

import graphs

pytestmark = pytest.mark.gpu


# ---- the oracle ---------------------------------------------------------------------------------
def oracle_row(keys, scores, rp, col, min_size, width, max_vol):
    """the five steps for one row; returns dict(order, swept, size, cut, vol, phi, pcut, pvol, W)"""
    n, m = len(rp) - 1, int(rp[-1])
    ents = []
    for k, s in zip(keys, scores):
        k = int(k)
        if not 0 <= k < n:
            continue
        d = int(rp[k + 1] - rp[k])
        r = float(np.float64(s) / np.float64(max(d, 1)))  # one IEEE divide
        ents.append((-r, k, d))
    ents.sort(key=lambda e: (e[0], e[1]))  # r descending, key ascending
    ents = ents[:width]
    order, pvol, vol = [], [], 0
    for _, k, d in ents:
        if vol + d > max_vol:
            break
        vol += d
        order.append(k)
        pvol.append(vol)
    swept = len(order)
    rank = {k: i for i, k in enumerate(order)}
    hist = [0] * swept
    for i, k in enumerate(order):
        for b in col[rp[k]:rp[k + 1]]:
            j = rank.get(int(b) & 0x7fffffff)
            if j is not None:
                hist[max(i, j)] += 1
    pcut, internal = [], 0
    best = None
    for j in range(1, swept + 1):
        internal += hist[j - 1]
        cut = pvol[j - 1] - internal
        den = min(pvol[j - 1], m - pvol[j - 1])
        pcut.append(cut)
        if j >= min_size and den > 0 and (best is None or cut * best[2] < best[1] * den):
            best = (j, cut, den, pvol[j - 1])
    if best is None:
        size, bc, bv, phi = 0, 0, 0, float("inf")
    else:
        size, bc, bv, phi = best[0], best[1], best[3], best[1] / best[2]
    return dict(order=order, swept=swept, size=size, cut=bc, vol=bv, phi=phi, pcut=pcut, pvol=pvol, W=vol)


def check(res, rows, g, min_size, width, max_vol, profile=False):
    """every row of a SweepResult against the oracle of rows[i] = (keys, scores); returns sum W"""
    rp, col = g.row_ptr, g.col
    if max_vol is None:
        max_vol = int(rp[-1]) // 2
    assert res.order.shape == (len(rows), width) and res.order.dtype == np.int32
    cache, total = {}, 0
    for i, (ks, ss) in enumerate(rows):
        key = (tuple(int(k) for k in ks), tuple(float(s) for s in ss))
        if key not in cache:
            cache[key] = oracle_row(ks, ss, rp, col, min_size, width, max_vol)
        w = cache[key]
        total += w["W"]
        pad = [-1] * (width - w["swept"])
        assert [int(x) for x in res.order[i]] == w["order"] + pad, i
        assert (int(res.swept[i]), int(res.size[i]), int(res.cut[i]), int(res.vol[i])) == \
            (w["swept"], w["size"], w["cut"], w["vol"]), i
        assert np.float64(res.phi[i]).view(np.uint64) == np.float64(w["phi"]).view(np.uint64), i
        if profile:
            assert [int(x) for x in res.profile_cut[i]] == w["pcut"] + pad, i
            assert [int(x) for x in res.profile_vol[i]] == w["pvol"] + pad, i
        else:
            assert res.profile_cut is None and res.profile_vol is None
    return total


def slab_rows(slab, sources):
    ids, sc, lens = slab
    return [(ids[u, :lens[u]], sc[u, :lens[u]]) for u in sources]


def same(a, b):
    for f in ("order", "swept", "size", "cut", "vol", "profile_cut", "profile_vol"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), f
    assert np.array_equal(a.phi.view(np.uint64), b.phi.view(np.uint64))


# ---- the plans ----------------------------------------------------------------------------------
GRAPHS = {
    "rmat10": (lambda: ppr.rmat(10), 16, 64, 12),
    "sparse600": (lambda: ppr.Csr(*graphs.sparse_random(600, 3)), 16, 32, 12),
    "multi500": (lambda: ppr.Csr(*graphs.multigraph(500, 5)), 16, 32, 12),
    "layered16": (lambda: ppr.Csr(*graphs.layered(16, 4)), 16, 32, 12),
}
_plans = {}


def plan_of(name):
    if name not in _plans:
        make, K, L, it = GRAPHS[name]
        g = make()
        plan = ppr.GrankPlan(g, K, L, 0.85)
        plan.run(it, -1.0)
        _plans[name] = (g, plan, plan.fetch_slab())
    return _plans[name]


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for _, plan, _ in _plans.values():
        plan.close()
    _plans.clear()


# ---- 1. the definition --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_definition(name):
    g, plan, slab = plan_of(name)
    L = plan.L
    everyone = list(range(g.n))
    rng = np.random.default_rng(11)
    some = [int(u) for u in rng.integers(0, g.n, size=40)]
    some += some[:5] + [some[0]] * 3 + [0, g.n - 1]
    for sources, src_arg in ((everyone, None), (some, some)):
        rows = slab_rows(slab, sources)
        st = {}
        res = plan.sweep(src_arg, stats=st)
        total = check(res, rows, g, 1, L, None)
        assert st["edges"] == total
        assert st["wave_sources"] + st["wg_sources"] + st["slice_sources"] == len(sources)
        res = plan.sweep(src_arg, min_size=3, max_size=7, max_vol=64, profile=True)
        check(res, rows, g, 3, 7, 64, profile=True)
        res = plan.sweep(src_arg, profile=True)
        check(res, rows, g, 1, L, None, profile=True)
    res = plan.sweep()
    none = int((res.size == 0).sum())
    assert np.all(np.isposinf(res.phi[res.size == 0])) and np.all(res.cut[res.size == 0] == 0)
    if name == "sparse600":
        assert none == 30  # (dangling sources: a one-entry row of volume 0 has no admissible prefix)
        deg = np.diff(g.row_ptr)
        assert np.all(deg[res.size == 0] == 0)
    if name == "layered16":  # one mass and one degree per layer: ties decided by the id rule alone
        ids, sc, lens = slab
        for u in range(g.n):
            k, s = ids[u, :lens[u]], sc[u, :lens[u]]
            assert all(len(set(s[(k // 16 == lay) & (k != u)])) <= 1 for lay in range(4))
            assert len(set(s)) < len(s)


# ---- 2. the tiers, the slices, the chunks, the order of the sources -----------------------------
def test_tier_independence(monkeypatch):
    g, plan, slab = plan_of("multi500")
    sources = list(range(g.n))
    rows = slab_rows(slab, sources)
    st = {}
    base = plan.sweep(profile=True, stats=st)
    total = check(base, rows, g, 1, plan.L, None, profile=True)
    assert st["edges"] == total
    deg = np.diff(g.row_ptr)
    assert deg[0] == 3003
    hubbed = [i for i in sources if 0 in base.order[i, :base.swept[i]]]
    assert hubbed  # the degree-3003 member is swept: at 1024 edges per slice it spans >= 3 slices
    big = 1 << 30
    forced = {"wave": dict(PPR_SW_WAVE_MAX=big), "wg": dict(PPR_SW_WAVE_MAX=0, PPR_SW_WG_MAX=big),
              "slice": dict(PPR_SW_WAVE_MAX=0, PPR_SW_WG_MAX=0, PPR_SW_SLICE=1024)}
    for tier, env in forced.items():
        for extra in ({}, dict(PPR_SW_CHUNK=7)):
            with monkeypatch.context() as mp:
                for k, v in {**env, **extra}.items():
                    mp.setenv(k, str(v))
                st = {}
                res = plan.sweep(profile=True, stats=st)
                same(res, base)
                assert st[tier + "_sources"] == g.n and st["edges"] == total
                assert st["chunks"] == ((g.n + 6) // 7 if extra else 1)
                rev = plan.sweep(sources[::-1], profile=True, stats=st)
                assert st[tier + "_sources"] == g.n and st["edges"] == total
            for f in ("order", "swept", "size", "cut", "vol", "profile_cut", "profile_vol"):
                assert np.array_equal(getattr(rev, f)[::-1], getattr(base, f)), (tier, f)
            assert np.array_equal(rev.phi[::-1].view(np.uint64), base.phi.view(np.uint64))


# ---- 3. it finds communities --------------------------------------------------------------------
def ring_of_cliques(ncl=8, size=16, bridges=2, seed=1):
    """complete cliques joined to the next in a ring by random undirected bridges (symmetric CSR)"""
    rng = np.random.default_rng(seed)
    lists = [[c * size + j for j in range(size) if j != i] for c in range(ncl) for i in range(size)]
    for c in range(ncl):
        for _ in range(bridges):
            a = c * size + int(rng.integers(size))
            b = ((c + 1) % ncl) * size + int(rng.integers(size))
            lists[a].append(b)
            lists[b].append(a)
    return ppr.Csr(*graphs._csr(lists))


def test_finds_communities():
    g = ring_of_cliques()
    plan = ppr.GrankPlan(g, 16, 64, 0.85)
    plan.run(20, -1.0)
    deg = np.diff(g.row_ptr)
    for c in range(8):
        members = list(range(c * 16, c * 16 + 16))
        res = plan.sweep(members, max_vol=3 * int(deg[members].sum()) // 2)
        for i, u in enumerate(members):
            assert sorted(int(v) for v in res.sets()[i]) == members, u
    d = plan.sweep([0, 17], max_vol=3 * int(deg[:16].sum()) // 2).to_dicts(g)  # (both cliques have that volume)
    assert sorted(d[0]) == list(range(16)) and sorted(d[1]) == list(range(16, 32))
    plan.close()


# ---- 4. vectors ---------------------------------------------------------------------------------
def test_vectors():
    g, plan, slab = plan_of("rmat10")
    rng = np.random.default_rng(4)
    seeds = [[int(u) for u in rng.integers(0, g.n, size=1 + q % 5)] for q in range(60)]
    qr = plan.query(seeds, 32)
    rows = [(qr.ids[q, :qr.lens[q]], qr.scores[q, :qr.lens[q]]) for q in range(len(seeds))]
    for kw in (dict(), dict(min_size=2, max_size=9, max_vol=500, profile=True)):
        res = plan.sweep_vectors(qr, **kw)
        check(res, rows, g, kw.get("min_size", 1), kw.get("max_size", 32), kw.get("max_vol"), kw.get("profile", False))
    # the slab's own rows as vectors: the same bits as the resident sweep
    sources = [int(u) for u in rng.integers(0, g.n, size=100)] + [0, 0, g.n - 1]
    ids, sc, lens = slab
    for kw in (dict(), dict(min_size=2, max_size=20, max_vol=300, profile=True)):
        same(plan.sweep_vectors(ids[sources], sc[sources], lens[sources], **kw), plan.sweep(sources, **kw))
    # a row's end found from its -1 padding
    same(plan.sweep_vectors(ids[sources], sc[sources]), plan.sweep(sources))


# ---- 5. wide rows -------------------------------------------------------------------------------
def test_wide_rows():
    g = ppr.rmat(11)
    plan = ppr.GrankPlan(g, 16, 2048, 0.85)
    plan.run(3, -1.0)
    slab = plan.fetch_slab()
    lens = slab[2]
    assert lens.max() > 1024
    rng = np.random.default_rng(5)
    sources = [int(u) for u in np.argsort(lens)[-24:]] + [int(u) for u in rng.integers(0, g.n, size=40)]
    rows = slab_rows(slab, sources)
    st = {}
    res = plan.sweep(sources, stats=st)
    assert st["edges"] == check(res, rows, g, 1, 2048, None)
    vec = plan.sweep_vectors(slab[0][sources], slab[1][sources], lens[sources], max_size=4096)
    same(vec, res)
    plan.close()


def test_widest_vectors(monkeypatch):
    """4096 distinct members in one row (the 8192-slot table) with the whole graph as the cap"""
    g = ppr.rmat(13)
    plan = ppr.GrankPlan(g, 16, 16, 0.85)  # (never run: the vectors need only its graph)
    m = int(g.row_ptr[-1])
    rng = np.random.default_rng(6)
    ids = np.stack([rng.permutation(g.n)[:4096] for _ in range(3)]).astype(np.int32)
    sc = rng.random((3, 4096)) * np.diff(g.row_ptr)[ids].clip(1)  # (spread r over members of every degree)
    sc[1, ::3] = 0.0
    lens = np.array([4096, 4096, 3000], dtype=np.int32)
    rows = [(ids[i, :lens[i]], sc[i, :lens[i]]) for i in range(3)]
    st = {}
    res = plan.sweep_vectors(ids, sc, lens, max_vol=m, profile=True, stats=st)
    assert st["edges"] == check(res, rows, g, 1, 4096, m, profile=True)
    assert res.swept.max() > 3072 and st["wg_sources"] + st["slice_sources"] == 3
    for k, v in dict(PPR_SW_WAVE_MAX=0, PPR_SW_WG_MAX=0, PPR_SW_SLICE=5000).items():
        monkeypatch.setenv(k, str(v))
    sl = plan.sweep_vectors(ids, sc, lens, max_vol=m, profile=True, stats=st)
    assert st["slice_sources"] == 3
    same(sl, res)
    plan.close()


# ---- 6. edges of the contract -------------------------------------------------------------------
def test_contract_edges():
    g, plan, slab = plan_of("rmat10")
    before = plan.fetch()
    empty = plan.sweep([])
    assert empty.order.shape == (0, plan.L) and empty.size.shape == (0,)
    assert plan.sweep_vectors(np.zeros((0, 8), dtype=np.int32), np.zeros((0, 8))).order.shape == (0, 8)
    # a cap below the first member's degree: nothing is swept
    lg, lplan, lslab = plan_of("layered16")  # (every degree is 16)
    res = lplan.sweep(max_vol=15, profile=True)
    check(res, slab_rows(lslab, range(lg.n)), lg, 1, lplan.L, 15, profile=True)
    assert np.all(res.swept == 0) and np.all(res.size == 0) and np.all(res.order == -1) and np.all(np.isposinf(res.phi))
    assert np.all(res.profile_cut == -1) and np.all(res.profile_vol == -1)
    deg = np.diff(g.row_ptr)
    sources = [u for u in range(g.n) if deg[u] >= 2][:50]
    rows = slab_rows(slab, sources)
    # min_size above what was swept
    res = plan.sweep(sources, min_size=plan.L, max_vol=200)
    check(res, rows, g, plan.L, plan.L, 200)
    assert np.all(res.swept < plan.L) and np.all(res.size == 0)
    # profiles off and on: the same answer
    off, on = plan.sweep(sources), plan.sweep(sources, profile=True)
    assert off.profile_cut is None and on.profile_cut.shape == (len(sources), plan.L)
    on.profile_cut = on.profile_vol = None
    same(off, on)
    # nothing was written into the plan: the top-K is unchanged, and the plan runs again like a fresh one
    after = plan.fetch()
    assert np.array_equal(before.ids, after.ids) and np.array_equal(before.scores.view(np.uint64), after.scores.view(np.uint64))
    assert np.array_equal(before.lens, after.lens)
    s2 = plan.fetch_slab()
    assert all(np.array_equal(a, b) for a, b in zip(slab, s2))
    plan.run(5, -1.0)
    again = plan.fetch()
    fresh = ppr.GrankPlan(g, 16, 64, 0.85)
    fresh.run(5, -1.0)
    want = fresh.fetch()
    fresh.close()
    assert np.array_equal(again.ids, want.ids) and np.array_equal(again.scores.view(np.uint64), want.scores.view(np.uint64))
    _, K, L, it = GRAPHS["rmat10"]
    plan.run(it, -1.0)  # (the module's other tests read this plan at its first state)
    assert all(np.array_equal(a, b) for a, b in zip(slab, plan.fetch_slab()))


def test_hot_encoded_ids_and_slot_rule(monkeypatch):
    """rows that hold hot-tagged ids (a chain-mode run) are decoded; the current row follows the slot
    rule of fetch_slab after 1, 2 and 3 iterations and for an earlier iteration count on request"""
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
        check(plan.sweep(profile=True), slab_rows(plan.fetch_slab(), range(g.n)), g, 1, 32, None, profile=True)
        plan.close()
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    src = [int(u) for u in np.random.default_rng(9).integers(0, g.n, size=200)]
    for it in (1, 2, 3):
        plan.run(it, -1.0)
        check(plan.sweep(src), slab_rows(plan.fetch_slab(), src), g, 1, 32, None)
    check(plan.sweep(src, iterations_run=2), slab_rows(plan.fetch_slab(2), src), g, 1, 32, None)
    plan.close()


# ---- 7. refusals --------------------------------------------------------------------------------
SENT = -77


def raw_call(plan, vectors, S=None, sources="all", min_size=1, max_size=0, max_vol=0, flags=0, width=None, prof=(False, False),
             p=None, it=None, rows=None, nulls=()):
    """the C call on sentinel-filled outputs; returns (code, outputs)"""
    n = plan.csr.n
    L = _lib.lib()
    if vectors:
        ids, sc, ln = rows
        R = ids.shape[0] if S is None else S
        W = ids.shape[1]
    else:
        src = None if isinstance(sources, str) else np.ascontiguousarray(sources, dtype=np.int32)
        R = (n if src is None else len(src)) if S is None else S
        W = plan.L
    w = width if width is not None else max(1, min(max_size if max_size else W, 4096))
    rr = max(R, 1)
    outs = dict(order=np.full((rr, w), SENT, np.int32), swept=np.full(rr, SENT, np.int32), size=np.full(rr, SENT, np.int32),
                cut=np.full(rr, SENT, np.int64), vol=np.full(rr, SENT, np.int64), phi=np.full(rr, float(SENT)),
                pc=np.full((rr, w), SENT, np.int64), pv=np.full((rr, w), SENT, np.int64))
    ptr = {k: (None if k in nulls else _lib.ptr(v)) for k, v in outs.items()}
    tail = (min_size, max_size, max_vol, flags, ptr["order"], ptr["swept"], ptr["size"], ptr["cut"], ptr["vol"], ptr["phi"],
            ptr["pc"] if prof[0] else None, ptr["pv"] if prof[1] else None, None)
    handle = plan._p if p is None else p
    if vectors:
        rc = L.ppr_grank_plan_sweep_vectors(handle, R, W, None if "ids" in nulls else _lib.ptr(ids),
                                            None if "scores" in nulls else _lib.ptr(sc),
                                            None if "lens" in nulls else _lib.ptr(ln), *tail)
    else:
        rc = L.ppr_grank_plan_sweep(handle, plan.iterations_run if it is None else it, R, _lib.ptr(src), *tail)
    return rc, outs


def untouched(outs):
    return all(np.all(v == SENT) for v in outs.values())


def test_refusals():
    g, plan, slab = plan_of("rmat10")
    n, L, m = g.n, plan.L, int(g.row_ptr[-1])
    ARG, RANGE, SOURCE = 1, 11, 12
    some = [1, 2, 3]
    cases = [
        (ARG, dict(S=-1, sources=some)),
        (ARG, dict(sources="all", S=n - 1)),                      # NULL sources with S != n
        (ARG, dict(sources=some, min_size=0)),
        (ARG, dict(sources=some, min_size=L + 1)),
        (ARG, dict(sources=some, min_size=6, max_size=5)),
        (ARG, dict(sources=some, max_vol=-1)),
        (ARG, dict(sources=some, max_vol=m + 1)),
        (ARG, dict(sources=some, prof=(True, False))),
        (ARG, dict(sources=some, prof=(False, True))),
        (ARG, dict(sources=some, flags=1)),
        (ARG, dict(sources=some, flags=1 << 31)),
        (ARG, dict(sources=some, it=-1)),
        (ARG, dict(sources=some, p=0)),                           # a null plan
        (RANGE, dict(sources=some, max_size=4097, width=8)),
        (SOURCE, dict(sources=[1, n, 2])),
        (SOURCE, dict(sources=[-1])),
    ] + [(ARG, dict(sources=some, nulls=(k,))) for k in ("order", "swept", "size", "cut", "vol", "phi")]
    for want, kw in cases:
        rc, outs = raw_call(plan, False, **kw)
        assert rc == want, kw
        assert untouched(outs), kw
    # vectors
    ids = np.array([[5, 9, 2, -1], [7, 1, -1, -1]], dtype=np.int32)
    sc = np.array([[0.5, 0.25, 0.125, 0.0], [0.5, 0.5, 0.0, 0.0]])
    ln = np.array([3, 2], dtype=np.int32)

    def mod(idx=None, val=None, what="ids"):
        a = {"ids": ids.copy(), "sc": sc.copy(), "ln": ln.copy()}
        if idx is not None:
            a[what][idx] = val
        return a["ids"], a["sc"], a["ln"]
    wide = (np.zeros((1, 4097), np.int32), np.zeros((1, 4097)), np.ones(1, np.int32))
    vcases = [
        (0, dict(rows=mod())),
        (ARG, dict(rows=mod(0, 5, "ln"))),                        # a length above width_in
        (ARG, dict(rows=mod(1, -1, "ln"))),
        (ARG, dict(rows=mod((0, 1), -0.5, "sc"))),
        (ARG, dict(rows=mod((1, 0), float("nan"), "sc"))),
        (ARG, dict(rows=mod((1, 1), float("inf"), "sc"))),
        (ARG, dict(rows=mod((0, 2), 5, "ids"))),                  # a repeated id within a row
        (SOURCE, dict(rows=mod((0, 1), n, "ids"))),
        (SOURCE, dict(rows=mod((1, 0), -3, "ids"))),
        (RANGE, dict(rows=wide, width=8)),
        (RANGE, dict(rows=mod(), max_size=4097)),
        (ARG, dict(rows=mod(), min_size=0)),
        (ARG, dict(rows=mod(), min_size=5)),                      # above width_in
        (ARG, dict(rows=mod(), min_size=3, max_size=2)),
        (ARG, dict(rows=mod(), max_vol=m + 1)),
        (ARG, dict(rows=mod(), max_vol=-5)),
        (ARG, dict(rows=mod(), flags=2)),
        (ARG, dict(rows=mod(), prof=(True, False))),
        (ARG, dict(rows=mod(), S=-2)),
        (ARG, dict(rows=mod(), p=0)),
        (ARG, dict(rows=mod(), nulls=("ids",))),
        (ARG, dict(rows=mod(), nulls=("scores",))),
        (ARG, dict(rows=mod(), nulls=("lens",))),
        (ARG, dict(rows=mod(), nulls=("phi",))),
    ]
    for want, kw in vcases:
        rc, outs = raw_call(plan, True, **kw)
        assert rc == want, kw
        if want:
            assert untouched(outs), kw
    # an MC plan
    mc = ppr.MccpPlan(g, 16, 64, 0.85)
    rc, outs = raw_call(plan, False, sources=some, p=mc._p)
    assert rc == ARG and untouched(outs)
    rc, outs = raw_call(plan, True, rows=mod(), p=mc._p)
    assert rc == ARG and untouched(outs)
    mc.close()
    # the Python surface raises with the code
    with pytest.raises(ppr.PprError) as e:
        plan.sweep(some, min_size=0)
    assert e.value.code == ARG
    with pytest.raises(ppr.PprError) as e:
        plan.sweep(some, max_size=5000)
    assert e.value.code == RANGE
    with pytest.raises(ppr.PprError) as e:
        plan.sweep([n])
    assert e.value.code == SOURCE
