"""Feature propagation through a plan's resident baskets (GrankPlan.propagate / propagate_t,
ppr.propagate; include/ppr_hip.h) against its definition restated in exact arithmetic from the
fetched slab: entries in stored order (ascending hash_b of the key), fp64 fma chains from +0.0, the
transposed lists in ascending position cut into chunks of 512 whose partial sums are added in chunk
order, one rounding to the feature type (fp32, or bf16 straight from the fp64 value). Outputs are
compared as bit patterns."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

pytestmark = pytest.mark.gpu

CHUNK = 512
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
MB = {"f32": 23, "bf16": 7}


# ---- the oracle ---------------------------------------------------------------------------------
def fma(a, b, c):
    """fl(a * b + c), one rounding (Python 3.10 has no math.fma)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def round_bits(x, mb):
    """bit pattern of the fp64 value x rounded to nearest even in a type with 8 exponent and mb
    mantissa bits (23: fp32, 7: bf16), by integer arithmetic on the exact value"""
    sign = (1 << (mb + 8)) if math.copysign(1.0, x) < 0 else 0
    if x == 0.0:
        return sign
    fr = Fraction(abs(x))
    e = max(math.frexp(abs(x))[1] - 1, -126)
    q = fr / (Fraction(2) ** (e - mb))  # in units of the last place
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    bits = ((e + 126) << mb) + n  # (n carries the implicit bit of a normal value)
    return sign | min(bits, 0xff << mb)


def hash_b(keys):
    """the row order's hash (csrc/ppr_device.h hash_b), all 32 bits"""
    x = (np.asarray(keys, dtype=np.uint64) ^ np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x


def stored_rows(slab):
    """[(keys, scores)] per node in stored order, from fetch_slab's rows"""
    ids, sc, lens = slab
    rows = []
    for u in range(len(lens)):
        k, s = ids[u, :lens[u]], sc[u, :lens[u]]
        o = np.argsort(hash_b(k), kind="stable")
        rows.append(([int(x) for x in k[o]], [float(x) for x in s[o]]))
    return rows


def weights_of(row, normalize):
    ks, ss = row
    if not normalize:
        return ss
    W = 0.0
    for s in ss:
        W = W + s
    return [0.0 if W == 0.0 else s / W for s in ss]


def oracle_fwd(rows, X, sources, cols, normalize=False):
    """fp64 accumulators [S, len(cols)] of Z = B[sources] X"""
    acc = np.zeros((len(sources), len(cols)))
    for i, u in enumerate(sources):
        ks = rows[u][0]
        ws = [Fraction(w) for w in weights_of(rows[u], normalize)]
        for ci, c in enumerate(cols):
            a = 0.0
            for k, w in zip(ks, ws):
                a = float(w * Fraction(float(X[k, c])) + Fraction(a))
            acc[i, ci] = a
    return acc


def postings_of(rows, sources, normalize=False):
    """{key: [(position, weight)]} in ascending position"""
    post = {}
    for i, u in enumerate(sources):
        for k, w in zip(rows[u][0], weights_of(rows[u], normalize)):
            post.setdefault(k, []).append((i, w))
    return post


def oracle_t(rows, X, sources, n, cols, normalize=False):
    """fp64 totals [n, len(cols)] of Y = B[sources]^T X"""
    acc = np.zeros((n, len(cols)))
    for k, lst in postings_of(rows, sources, normalize).items():
        lw = [(i, Fraction(w)) for i, w in lst]
        for ci, c in enumerate(cols):
            total = None
            for b in range(0, len(lw), CHUNK):
                a = 0.0
                for i, w in lw[b:b + CHUNK]:
                    a = float(w * Fraction(float(X[i, c])) + Fraction(a))
                total = a if total is None else total + a
            acc[k, ci] = total
    return acc


def to_bits(acc, kind):
    return np.array([[round_bits(float(x), MB[kind]) for x in r] for r in acc], dtype=np.uint32).reshape(acc.shape)


def bits_of(t):
    t = t.detach()
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32)


def features(rng, rows, F, kind):
    """signed values with magnitudes in [2^-10, 2^10] and exact zeros, exact in bf16 (so one draw
    serves both types); returns (device tensor, its fp64 host copy)"""
    mag = np.exp2(rng.uniform(-10.0, 10.0, size=(rows, F)))
    x = mag * rng.choice([-1.0, 1.0], size=(rows, F))
    x[rng.random((rows, F)) < 0.1] = 0.0
    t = torch.tensor(x, dtype=torch.float64).to(torch.bfloat16)
    host = t.double().numpy()
    nz = host[host != 0.0]
    assert np.all(np.abs(nz) >= 2.0 ** -10) and np.all(np.abs(nz) <= 2.0 ** 10) and np.any(host == 0.0)
    return t.to(DTYPES[kind]).cuda(), host


def sample_cols(F):
    if F <= 16:
        return list(range(F))
    inner = np.random.default_rng(F).choice(np.arange(1, F - 1), size=14, replace=False)
    return [0] + sorted(int(c) for c in inner) + [F - 1]


def test_oracle_rounding():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.standard_normal(200) * np.exp2(rng.integers(-140, 130, size=200)),
                         [0.0, -0.0, 1.0, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** 128, 1 + 2.0 ** -24,
                          1 + 3 * 2.0 ** -24]])
    with np.errstate(over="ignore"):
        want = xs.astype(np.float32).view(np.uint32)
    assert [round_bits(float(x), 23) for x in xs] == [int(w) for w in want]
    # bf16 straight from the fp64 value: 1 + 2^-8 + 2^-30 lies above the tie (through fp32 it would fall on it)
    assert round_bits(1 + 2.0 ** -8 + 2.0 ** -30, 7) == 0x3f81
    assert round_bits(1 + 2.0 ** -8, 7) == 0x3f80 and round_bits(1 + 3 * 2.0 ** -8, 7) == 0x3f82
    assert fma(3.0, 1 + 2.0 ** -30, -3.0) == 3 * 2.0 ** -30


# ---- the base plan ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    g = ppr.rmat(10, seed=5)
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.run(6, -1.0)
    slab = plan.fetch_slab()
    rows = stored_rows(slab)
    # the stored order, once, against the raw rows
    it = plan.iterations_run
    sA, sB = ((it + 1) // 2) & 1, (it // 2) & 1
    raw = [None, None]
    for slot in (0, 1):
        ids = np.zeros((g.n, 32), dtype=np.int32)
        ln = np.zeros(g.n, dtype=np.int32)
        _lib.check(_lib.lib().ppr_plan_fetch_slot(plan._p, slot, _lib.ptr(ids), None, _lib.ptr(ln)))
        raw[slot] = (ids, ln)
    for u in range(g.n):
        ids, ln = raw[sB if plan.part[u] else sA]
        assert [int(x) for x in ids[u, :ln[u]]] == rows[u][0]
    yield g, plan, slab, rows
    plan.close()


def mixed_sources(g, slab, rng):
    lens = slab[2]
    dangling = np.nonzero(lens == 1)[0]
    assert len(dangling) > 10
    hub = int(np.argmax(np.diff(g.row_ptr)))
    src = [int(u) for u in rng.integers(0, g.n, size=10)]
    src += [src[0]] * 3 + [hub, hub]                      # repeats, the widest hub
    src += [int(u) for u in dangling[:9]]                 # dangling sources (one-entry rows)
    src += [int(np.argmax(lens)), 0, g.n - 1]
    return src


# ---- 1. forward, all sources --------------------------------------------------------------------
def test_forward_all_sources(base):
    g, plan, slab, rows = base
    F = 8
    acc = None
    for kind in ("f32", "bf16"):
        H, Hh = features(np.random.default_rng(1), g.n, F, kind)
        if acc is None:
            acc = oracle_fwd(rows, Hh, list(range(g.n)), list(range(F)))
        st = {}
        Z = plan.propagate(H, stats=st)
        assert Z.shape == (g.n, F) and Z.dtype == DTYPES[kind]
        assert np.array_equal(bits_of(Z), to_bits(acc, kind))
        esz = 4 if kind == "f32" else 2
        P = int(slab[2].sum())
        assert st["postings"] == P and st["passes"] == 1
        assert st["algo_bytes"] == P * (12 + F * esz) + g.n * F * esz + 8 * g.n


# ---- 2. forward shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 64, 100, 320])
def test_forward_shapes(base, F):
    g, plan, slab, rows = base
    rng = np.random.default_rng(20 + F)
    src = mixed_sources(g, slab, rng)
    cols = sample_cols(F)
    acc = None
    for kind in ("f32", "bf16"):
        H, Hh = features(np.random.default_rng(F), g.n, F, kind)
        if acc is None:
            acc = oracle_fwd(rows, Hh, src, cols)
        want = to_bits(acc, kind)
        Z = plan.propagate(H, src)
        assert np.array_equal(bits_of(Z)[:, cols], want)
        # only dangling sources; an empty batch
        dang = [int(u) for u in np.nonzero(slab[2] == 1)[0][:70]]
        Zd = plan.propagate(H, dang)
        wd = to_bits(oracle_fwd(rows, Hh, dang[:8], cols), kind)
        assert np.array_equal(bits_of(Zd)[:8, cols], wd)
        assert plan.propagate(H, []).shape == (0, F)
        # out= with a row stride above F (one that keeps the vector path and one that does not)
        for pad in (8, 5):
            full = torch.full((len(src), F + pad), float("nan"), dtype=DTYPES[kind], device="cuda")
            out = full[:, :F]
            assert plan.propagate(H, src, out=out) is out
            assert np.array_equal(bits_of(out)[:, cols], want)
            assert bool(torch.isnan(full[:, F:]).all())
            assert np.array_equal(bits_of(out), bits_of(Z))


# ---- 3. rows that are not 16-byte aligned -------------------------------------------------------
def test_unaligned_rows():
    g = ppr.rmat(10, seed=5)
    plan = ppr.GrankPlan(g, 16, 30, 0.85)
    plan.run(6, -1.0)
    rows = stored_rows(plan.fetch_slab())
    rng = np.random.default_rng(3)
    src = [int(u) for u in rng.integers(0, g.n, size=128)]
    for kind in ("f32", "bf16"):
        H, Hh = features(np.random.default_rng(30), g.n, 8, kind)
        assert np.array_equal(bits_of(plan.propagate(H, src)), to_bits(oracle_fwd(rows, Hh, src, list(range(8))), kind))
        G, Gh = features(np.random.default_rng(31), len(src), 4, kind)
        Y = plan.propagate_t(G, src)
        assert np.array_equal(bits_of(Y), to_bits(oracle_t(rows, Gh, src, g.n, list(range(4))), kind))
    plan.close()


# ---- 4. row normalisation -----------------------------------------------------------------------
def test_row_normalisation(base):
    g, plan, slab, rows = base
    rng = np.random.default_rng(4)
    src = mixed_sources(g, slab, rng) + [int(u) for u in rng.integers(0, g.n, size=64)]
    for kind in ("f32", "bf16"):
        H, Hh = features(np.random.default_rng(40), g.n, 4, kind)
        want = to_bits(oracle_fwd(rows, Hh, src, list(range(4)), normalize=True), kind)
        assert np.array_equal(bits_of(plan.propagate(H, src, normalize=True)), want)
        assert not np.array_equal(bits_of(plan.propagate(H, src)), want)
        G, Gh = features(np.random.default_rng(41), len(src), 4, kind)
        want = to_bits(oracle_t(rows, Gh, src, g.n, list(range(4)), normalize=True), kind)
        assert np.array_equal(bits_of(plan.propagate_t(G, src, normalize=True)), want)


# ---- 5. transposed ------------------------------------------------------------------------------
def test_transposed(base):
    """every node twice: the most frequent key's list takes three chunks and more, and the keys that
    sit in a single row have the shortest lists there are (two postings); a small batch afterwards
    has lists of exactly one posting and mostly untouched keys"""
    g, plan, slab, rows = base
    F = 4
    src = list(range(g.n)) * 2
    post = postings_of(rows, src)
    assert max(len(v) for v in post.values()) > 2 * CHUNK      # a list of at least 3 chunks
    assert sum(1 for v in post.values() if len(v) == 2) > 20   # (every node twice: the shortest lists)
    acc = None
    for kind in ("f32", "bf16"):
        G, Gh = features(np.random.default_rng(5), len(src), F, kind)
        if acc is None:
            acc = oracle_t(rows, Gh, src, g.n, list(range(F)))
        Y = torch.full((g.n, F), float("nan"), dtype=DTYPES[kind], device="cuda")
        st = {}
        assert plan.propagate_t(G, src, out=Y, stats=st) is Y
        assert np.array_equal(bits_of(Y), to_bits(acc, kind))
        P = 2 * int(slab[2].sum())
        esz = 4 if kind == "f32" else 2
        assert st["postings"] == P and st["passes"] == 1 and st["chunks"] >= len(post) + 2
        assert st["algo_bytes"] == P * (12 + F * esz) + g.n * F * esz + 8 * len(src)
    # a small batch: most keys have one posting, most rows of Y are untouched and come back as zeros
    small = [int(u) for u in np.nonzero(slab[2] == 1)[0][:40]] + [5, 5, 7]
    post = postings_of(rows, small)
    assert sum(1 for v in post.values() if len(v) == 1) > 20 and len(post) < g.n // 2
    for kind in ("f32", "bf16"):
        G, Gh = features(np.random.default_rng(6), len(small), F, kind)
        Y = torch.full((g.n, F), float("nan"), dtype=DTYPES[kind], device="cuda")
        plan.propagate_t(G, small, out=Y)
        got = bits_of(Y)
        assert np.array_equal(got, to_bits(oracle_t(rows, Gh, small, g.n, list(range(F))), kind))
        untouched = [k for k in range(g.n) if k not in post]
        assert len(untouched) > g.n // 2 and not got[untouched].any()
    # no sources at all: every row of Y is zero
    Y = torch.full((g.n, F), float("nan"), dtype=torch.float32, device="cuda")
    plan.propagate_t(torch.zeros((0, F), device="cuda"), [], out=Y)
    assert not bits_of(Y).any()


def test_transposed_wide(base, monkeypatch):
    """more than one column tile, a tail tile, lists of two chunks; and the column blocks that bound
    the partial rows (a budget of one byte: blocks of a single tile) give the same bits"""
    g, plan, slab, rows = base
    F = 320
    src = list(range(g.n))
    assert max(len(v) for v in postings_of(rows, src).values()) > CHUNK
    cols = sample_cols(F)
    acc = None
    for kind in ("f32", "bf16"):
        G, Gh = features(np.random.default_rng(55), len(src), F, kind)
        if acc is None:
            acc = oracle_t(rows, Gh, src, g.n, cols)
        want = bits_of(plan.propagate_t(G))
        assert np.array_equal(want[:, cols], to_bits(acc, kind))
        monkeypatch.setenv("PPR_PROP_PART_BYTES", "1")
        assert np.array_equal(bits_of(plan.propagate_t(G, src)), want)
        monkeypatch.setenv("PPR_PROP_V", "1")  # tiles of 64 columns: five blocks
        assert np.array_equal(bits_of(plan.propagate_t(G, src)), want)
        monkeypatch.delenv("PPR_PROP_V")
        monkeypatch.delenv("PPR_PROP_PART_BYTES")


# ---- 6. independence ----------------------------------------------------------------------------
def test_independence(base, monkeypatch):
    g, plan, slab, rows = base
    src = list(range(g.n)) * 2
    for kind in ("f32", "bf16"):
        G, _ = features(np.random.default_rng(60), len(src), 8, kind)
        st = {}
        want = bits_of(plan.propagate_t(G, src, stats=st))
        assert st["passes"] == 1
        monkeypatch.setenv("PPR_PROP_ENTRIES", "1")  # E = max(1, S): a dozen key-range passes
        st = {}
        got = bits_of(plan.propagate_t(G, src, stats=st))
        monkeypatch.delenv("PPR_PROP_ENTRIES")
        assert st["passes"] >= 4 and st["postings"] == 2 * int(slab[2].sum())
        assert np.array_equal(got, want)
        for knob in ("PPR_PROP_V", "PPR_PROP_HOST_PLAN"):  # one column per lane; chunk tasks built on the host
            monkeypatch.setenv(knob, "1")
            assert np.array_equal(bits_of(plan.propagate_t(G, src)), want)
            monkeypatch.delenv(knob)
        # forward: the lane geometry both ways, and a batch split into two calls
        for F in (8, 320):
            H, _ = features(np.random.default_rng(61), g.n, F, kind)
            fsrc = mixed_sources(g, slab, np.random.default_rng(62)) * 3
            want_f = bits_of(plan.propagate(H, fsrc))
            for knob in ("PPR_PROP_PACK", "PPR_PROP_V"):
                monkeypatch.setenv(knob, "0" if knob == "PPR_PROP_PACK" else "1")
                assert np.array_equal(bits_of(plan.propagate(H, fsrc)), want_f)
                monkeypatch.delenv(knob)
            cut = len(fsrc) // 3 + 1
            two = np.concatenate([bits_of(plan.propagate(H, fsrc[:cut])), bits_of(plan.propagate(H, fsrc[cut:]))])
            assert np.array_equal(two, want_f)


# ---- 7. adjointness at a larger shape -----------------------------------------------------------
@pytest.mark.parametrize("kind,bound", [("f32", 2.0 ** -22), ("bf16", 2.0 ** -6)])
def test_adjointness(kind, bound):
    """<Z, G> = <H, Y> up to the output roundings: each side's only non-negligible error is one
    rounding per output element, relative 2^-24 (fp32) / 2^-8 (bf16) of a sum whose terms' absolute
    values add up to at most sum |w H G|; the fp64 chains add ~(L + chunks) 2^-53. Two sides, rounded
    up to a power of two: 2^-22 and 2^-6 of sum |w H G|."""
    g = ppr.rmat(12, seed=5)
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.run(6, -1.0)
    ids, sc, lens = plan.fetch_slab()
    rng = np.random.default_rng(7)
    src = rng.integers(0, g.n, size=2000)
    F = 64
    H, Hh = features(np.random.default_rng(70), g.n, F, kind)
    G, Gh = features(np.random.default_rng(71), len(src), F, kind)
    Z = plan.propagate(H, src).double().cpu().numpy()
    Y = plan.propagate_t(G, src).double().cpu().numpy()
    lhs, rhs = float((Z * Gh).sum()), float((Hh * Y).sum())
    w = np.where(np.arange(32)[None, :] < lens[src][:, None], sc[src], 0.0)       # [S, L]
    k = np.where(np.arange(32)[None, :] < lens[src][:, None], ids[src], 0)
    scale = float(np.einsum("sl,slf,sf->", w, np.abs(Hh)[k], np.abs(Gh)))
    print(f"adjointness {kind}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound = {bound * scale:.3e}")
    assert scale > 0 and abs(lhs - rhs) <= bound * scale
    plan.close()


# ---- 8. hot-tagged ids --------------------------------------------------------------------------
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
    rows = stored_rows(plan.fetch_slab())
    src = [int(u) for u in np.random.default_rng(8).integers(0, g.n, size=256)]
    for kind in ("f32", "bf16"):
        H, Hh = features(np.random.default_rng(80), g.n, 4, kind)
        assert np.array_equal(bits_of(plan.propagate(H, src)), to_bits(oracle_fwd(rows, Hh, src, list(range(4))), kind))
        G, Gh = features(np.random.default_rng(81), len(src), 4, kind)
        assert np.array_equal(bits_of(plan.propagate_t(G, src)),
                              to_bits(oracle_t(rows, Gh, src, g.n, list(range(4))), kind))
    plan.close()


# ---- 9. slot rule, no trace ---------------------------------------------------------------------
def test_slot_rule_and_no_trace():
    g = ppr.rmat(10, seed=5)
    src = [int(u) for u in np.random.default_rng(9).integers(0, g.n, size=100)]
    H, Hh = features(np.random.default_rng(90), g.n, 4, "f32")
    G, Gh = features(np.random.default_rng(91), len(src), 4, "f32")
    plan = ppr.GrankPlan(g, 16, 32, 0.85)
    plan.init()
    slab0 = plan.fetch_slab(0)
    rows0 = stored_rows(slab0)
    cols = list(range(4))
    assert np.array_equal(bits_of(plan.propagate(H, src, iterations_run=0)), to_bits(oracle_fwd(rows0, Hh, src, cols), "f32"))
    assert np.array_equal(bits_of(plan.propagate_t(G, src, iterations_run=0)),
                          to_bits(oracle_t(rows0, Gh, src, g.n, cols), "f32"))
    plan.run(5, -1.0)  # an odd iteration count
    slab5 = plan.fetch_slab()
    rows5 = stored_rows(slab5)
    assert not np.array_equal(slab0[1], slab5[1])
    assert np.array_equal(bits_of(plan.propagate(H, src)), to_bits(oracle_fwd(rows5, Hh, src, cols), "f32"))
    assert np.array_equal(bits_of(plan.propagate_t(G, src)), to_bits(oracle_t(rows5, Gh, src, g.n, cols), "f32"))
    # the calls leave no trace: the plan runs again like a fresh one
    plan.run(6, -1.0)
    again = plan.fetch()
    fresh = ppr.GrankPlan(g, 16, 32, 0.85)
    fresh.run(6, -1.0)
    want = fresh.fetch()
    assert np.array_equal(again.ids, want.ids) and np.array_equal(again.scores, want.scores)
    assert np.array_equal(again.lens, want.lens)
    plan.close()
    fresh.close()


# ---- 10. refusals -------------------------------------------------------------------------------
def test_refusals(base):
    g, plan, slab, rows = base
    n = g.n
    H = torch.zeros((n, 16), device="cuda")
    Z = torch.zeros((n, 16), device="cuda")
    L = _lib.lib()
    src = np.array([1, 2, 3], dtype=np.int32)

    def code(fn=L.ppr_grank_plan_propagate, p=None, S=3, sources=src, F=16, dt=0, flags=0, a=H.data_ptr(), lda=16,
             b=Z.data_ptr(), ldb=16):
        return fn(p or plan._p, plan.iterations_run, S, _lib.ptr(sources), F, dt, flags, a, lda, b, ldb, None)

    for fn in (L.ppr_grank_plan_propagate, L.ppr_grank_plan_propagate_t):
        assert code(fn) == 0
        assert code(fn, a=None) == 1 and code(fn, b=None) == 1      # PPR_ERR_ARG: null pointers
        assert code(fn, S=-1) == 1
        assert code(fn, S=3, sources=None) == 1                     # NULL sources with S != n
        assert code(fn, S=n, sources=None) == 0
        assert code(fn, lda=15) == 1 and code(fn, ldb=15) == 1      # a stride below F
        assert code(fn, dt=2) == 1 and code(fn, flags=2) == 1       # unknown dtype / flag bits
        assert code(fn, F=0) == 11 and code(fn, F=8193, lda=8193, ldb=8193) == 11   # PPR_ERR_RANGE
        assert code(fn, sources=np.array([1, n, 3], dtype=np.int32)) == 12          # PPR_ERR_SOURCE
        assert code(fn, sources=np.array([1, -1, 3], dtype=np.int32)) == 12
        mc = ppr.MccpPlan(g, 16, 32, 0.85)
        assert code(fn, p=mc._p) == 1                               # an MC plan
        mc.close()
    # the wrapper refuses before any call
    assert plan.device == torch.cuda.current_device()
    with pytest.raises(ValueError):
        plan.propagate(torch.zeros((n, 4)))                         # not on the plan's device
    with pytest.raises(TypeError):
        plan.propagate(torch.zeros((n, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        plan.propagate(torch.zeros((n, 4), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        plan.propagate(torch.zeros((n, 4, 1), device="cuda"))       # not 2-D
    with pytest.raises(ValueError):
        plan.propagate(torch.zeros((n - 1, 4), device="cuda"))      # rows != n
    with pytest.raises(ValueError):
        plan.propagate_t(torch.zeros((4, 4), device="cuda"), [1, 2, 3])   # rows != S
    with pytest.raises(ValueError):
        plan.propagate(torch.zeros((4, n), device="cuda").t())      # rows not contiguous
    with pytest.raises(ValueError):
        plan.propagate(H, [1, 2], out=torch.zeros((3, 16), device="cuda"))
    with pytest.raises(TypeError):
        plan.propagate(H, [1, 2], out=torch.zeros((2, 16), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ppr.PprError):
        plan.propagate(H, [1, n])
    # and the plan answers afterwards
    Hr, Hh = features(np.random.default_rng(100), n, 4, "f32")
    assert np.array_equal(bits_of(plan.propagate(Hr, [3, 4])), to_bits(oracle_fwd(rows, Hh, [3, 4], list(range(4))), "f32"))


# ---- 11. autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_autograd(base, kind):
    g, plan, slab, rows = base
    src = mixed_sources(g, slab, np.random.default_rng(11))
    H, _ = features(np.random.default_rng(110), g.n, 8, kind)
    C, _ = features(np.random.default_rng(111), len(src), 8, kind)
    for normalize in (False, True):
        Hg = H.clone().requires_grad_()
        Z = ppr.propagate(plan, Hg, src, normalize)
        assert Z.requires_grad
        assert np.array_equal(bits_of(Z), bits_of(plan.propagate(H, src, normalize)))
        Z.backward(C)
        assert np.array_equal(bits_of(Hg.grad), bits_of(plan.propagate_t(C, src, normalize)))
        Hg = H.clone().requires_grad_()
        ppr.propagate(plan, Hg, src, normalize).sum().backward()
        ones = torch.ones((len(src), 8), dtype=DTYPES[kind], device="cuda")
        assert np.array_equal(bits_of(Hg.grad), bits_of(plan.propagate_t(ones, src, normalize)))
    # every node, in order
    Hg = H.clone().requires_grad_()
    Ca, _ = features(np.random.default_rng(112), g.n, 8, kind)
    ppr.propagate(plan, Hg).backward(Ca)
    assert np.array_equal(bits_of(Hg.grad), bits_of(plan.propagate_t(Ca)))
