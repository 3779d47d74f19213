"""Batched exact PPR on the GPU against the reference's pprSingleSource
(include/internal/pprSingleSource.h:28-75) recorded in the golden fixtures: every score within
1e-12 (the per-node summation order differs from the reference's map order, so not bit for bit),
the same keys wherever scores are not tied.

Below the fixture tests: the kernels against tests/exact_ref.py, the long-double restatement that
tests/test_exact_ref_host.py pins to the same fixtures, at the batch widths, graph sizes, stop
iterations, top-K cuts and gather shapes the fixtures do not reach. The tolerance is the engine's
contract, 1e-12 absolute on every score of the whole vector, zeros included."""
import ctypes
import functools

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
import exact_ref
import graphs
from approximated_personalized_pagerank_amd import _lib
from exact_ref import check_rows
from helpers import load

pytestmark = pytest.mark.gpu

FULL = ["g5_ring100_full", "g5_instar_full", "g5_instar_loop_full", "g5_instar_all_full", "g5_random5000_full",
        "g5_complete_full", "m2_random100_full"]


@pytest.mark.parametrize("name", FULL)
def test_gpu_exact_ppr_vs_reference_full_rows(name):
    """100 iterations, no tolerance stop, every source of a 100-node graph, whole vectors"""
    f = load(name)
    z = f["z"]
    g = ppr.Csr(f["rp"], f["col"])
    n = g.n
    ex = ppr.ExactPPR(g, np.arange(n), 0.85, device=0)
    it = ex.run(100, -1.0)
    assert (it == 100).all()
    ids, sc, ln = ex.topk(n)
    ex.close()
    assert np.array_equal(ln, z["pprss_cnt"])
    check_rows(ids, sc, ln, z["pprss_ids"], z["pprss_scores"], z["pprss_cnt"])


@pytest.mark.parametrize("name", ["g3_rmat12_k16_l32", "g3_rmat14_k32_l64", "g3_rmat14_k64_l128"])
def test_gpu_exact_ppr_vs_reference_sampled(name):
    """the reference harness's call pprSingleSource(g, 100, .85, 1e-4, v) (benchmarkAlgorithm.h:91)
    for 200 sampled sources of RMAT-12/14, top K + 32 entries"""
    f = load(name)
    z = f["z"]
    g = ppr.Csr(f["rp"], f["col"])
    src = z["pprss_src"]
    kk = z["pprss_ids"].shape[1]
    ex = ppr.ExactPPR(g, src, 0.85, device=0)
    ex.run(100, 1e-4)
    ids, sc, ln = ex.topk(kk)
    ex.close()
    rc = np.minimum(z["pprss_cnt"], kk)
    assert np.array_equal(np.minimum(ln, kk), rc)
    check_rows(ids, sc, np.minimum(ln, kk), z["pprss_ids"], z["pprss_scores"], rc)


def test_gpu_benchmark_algorithm_on_grank():
    """benchmarkAlgorithm over a GPU grank result: the engine's quality on RMAT-12 K16/L32 matches
    the oracle-side figure of tests/test_parity_p34.py (>= the reference's own 0.90, minus 0.01)"""
    f = load("g3_rmat12_k16_l32")
    g = ppr.Csr(f["rp"], f["col"])
    r = ppr.grank_csr(g, f["K"], f["L"], f["iters"], f["damping"], f["tol"], part=f["part"], device=0)
    res = {v: {int(i): float(s) for i, s in zip(r.ids[v, :r.lens[v]], r.scores[v, :r.lens[v]])} for v in range(g.n)}
    q = ppr.benchmark_algorithm(res, g, 400, True, seed=1, device=0)
    assert q["jaccard average"] >= 0.89, q
    assert 0.0 < q["kendall average"] <= 1.0 and q["average map size"] == pytest.approx(16.0, abs=0.5), q


# ---- the kernels against the long-double restatement (tests/exact_ref.py) ----

TOL = 1e-12     # the engine's contract (csrc/exact_ppr.hip header, include/ppr_hip.h): absolute, scores <= 1
LD = np.longdouble
D = 0.85


def csr(n, seed):
    return ppr.Csr(*graphs.sparse_random(n, seed))


def dense(ex):
    """a handle's whole [n, S] score matrix, zeros included, through gather(arange(n))"""
    n, S = ex.csr.n, len(ex.sources)
    return np.ascontiguousarray(ex.gather(np.tile(np.arange(n, dtype=np.int32), (S, 1))).T)


def err(x, ref_scores):
    return float(np.abs(x.astype(LD) - ref_scores).max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run_fresh(g, src, damping, iterations, tol):
    ex = ppr.ExactPPR(g, src, damping, device=0)
    it = ex.run(iterations, tol)
    x = dense(ex)
    ex.close()
    return it, x


def mixed_sources(g, S, seed):
    """S distinct sources, most of them ordinary nodes; dangling nodes (they stop at iteration 2) at
    positions 3, 33, 63, ... (63 is the last lane of a wave) and nodes whose successors are all
    dangling (they stop at 3) at 10, 60, 110"""
    rng = np.random.default_rng(seed)
    deg = g.degrees()
    dang = np.flatnonzero(deg == 0)
    alld = np.array([v for v in np.flatnonzero(deg > 0)
                     if (deg[g.col[g.row_ptr[v]:g.row_ptr[v + 1]]] == 0).all()], dtype=np.int64)
    src = rng.choice(np.setdiff1d(np.flatnonzero(deg > 0), alld), S, replace=False)
    for i, p in enumerate(range(3, S, 30)):
        src[p] = dang[i]
    for i, p in enumerate(range(10, S, 50)):
        if i < len(alld):
            src[p] = alld[i]
    return src.astype(np.int32)


def diffs_clear_of(ref, tol, margin=1e-6):
    """the stop decision `diff >= tol` of every source at every iteration is not a matter of rounding:
    the reference's diff is further than margin * tol from tol (the kernels' diff, a sum of n terms
    <= 1 in double, is within ~1e-13 of it)"""
    d = ref.diffs[~np.isnan(ref.diffs.astype(np.float64))]
    return float(np.abs(d / LD(tol) - 1).min()) > margin


@functools.lru_cache(maxsize=None)
def small():
    """401 nodes, 130 sources (position 70 repeats position 5), 30 iterations, nothing stops"""
    g = csr(401, 11)
    src = mixed_sources(g, 130, 1)
    src[70] = src[5]
    return g, src, exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 30, -1.0)


@functools.lru_cache(maxsize=None)
def small_gpu():
    g, src, _ = small()
    ex = ppr.ExactPPR(g, src, D, device=0)
    it = ex.run(30, -1.0)
    return ex, it, dense(ex)


@functools.lru_cache(maxsize=None)
def small_stopped():
    g, src, _ = small()
    return exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 100, 1e-4)


@functools.lru_cache(maxsize=None)
def big():
    """8200 nodes (the pull grid's 4096 waves take a third lap), 130 sources, the harness's own call:
    100 iterations, 1e-4"""
    g = csr(8200, 3)
    src = mixed_sources(g, 130, 3)
    return g, src, exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 100, 1e-4)


@functools.lru_cache(maxsize=None)
def big_gpu():
    g, src, _ = big()
    ex = ppr.ExactPPR(g, src, D, device=0)
    it = ex.run(100, 1e-4)
    return ex, it, dense(ex)


# -- a. batch widths and grid laps

@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_gpu_exact_batch_widths(S):
    """one lane, a wave short of one lane, a full wave, one lane into the second pass of the
    `s0 += WAVE` loop, and a third pass that is nearly empty"""
    g, src, ref = small()
    it, x = run_fresh(g, src[:S], D, 30, -1.0)
    assert (it == 30).all() and x.shape == (g.n, S)
    assert err(x, ref.scores[:, :S]) <= TOL


def test_gpu_exact_repeated_and_dangling_sources():
    g, src, ref = small()
    _, it, x = small_gpu()
    assert src[70] == src[5] and same_bits(x[:, 70], x[:, 5])
    dang = np.flatnonzero(g.degrees()[src] == 0)
    assert len(dang) >= 4
    for p in dang:
        col = np.zeros(g.n)
        col[src[p]] = 1.0 - D
        assert same_bits(x[:, p], col), p
    assert err(x, ref.scores) <= TOL


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8200])
def test_gpu_exact_grid_laps(n):
    """the grid-stride over targets around its first second lap (4096 waves) and into a third"""
    g = csr(n, n)
    src = mixed_sources(g, 65, n)
    ref = exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 20, -1.0)
    it, x = run_fresh(g, src, D, 20, -1.0)
    assert (it == 20).all()
    assert err(x, ref.scores) <= TOL


@pytest.mark.parametrize("damping", [0.85, 0.3, 1.0])
def test_gpu_exact_multigraph_and_mass(damping):
    """repeated edges count once per repetition, doubled self-loops, a 303-edge hub; no node is
    dangling, so every column keeps a mass of exactly 1: (1 - d) + d * 1"""
    g = ppr.Csr(*graphs.multigraph(400, 5, hub=300))
    assert g.degrees().min() > 0
    src = np.array([0, 1, 2, 3, 7, 14, 21, 200, 398, 399], dtype=np.int32)
    ref = exact_ref.exact_ppr(g.row_ptr, g.col, src, damping, 25, -1.0)
    assert np.abs(ref.scores.sum(axis=0) - 1).max() <= 1e-16
    it, x = run_fresh(g, src, damping, 25, -1.0)
    assert (it == 25).all()
    assert err(x, ref.scores) <= TOL
    assert np.abs(x.astype(LD).sum(axis=0) - 1).max() <= TOL


# -- b. the per-source stop rule

def test_gpu_exact_stop_rule_per_source():
    """every source stops at its own iteration (dangling sources at 2, sources that feed only
    dangling nodes at 3, ordinary ones in the tens) and its column is the reference's at that stop:
    a column that kept iterating, or stopped with the batch, is off by far more than 1e-12"""
    g, src, ref = big()
    assert diffs_clear_of(ref, 1e-4)
    stops = set(ref.iters.tolist())
    assert len(stops) >= 3 and {2, 3} <= stops and max(stops) < 100
    _, it, x = big_gpu()
    assert np.array_equal(it, ref.iters)
    worst = np.abs(x.astype(LD) - ref.scores).max(axis=0)
    assert worst.max() <= TOL, (int(worst.argmax()), float(worst.max()))


def test_gpu_exact_iteration_cap_and_stop_rule_small():
    g, src, _ = small()
    ref = small_stopped()
    assert diffs_clear_of(ref, 1e-4) and len(set(ref.iters.tolist())) >= 3
    it, x = run_fresh(g, src, D, 100, 1e-4)
    assert np.array_equal(it, ref.iters) and err(x, ref.scores) <= TOL
    cap = exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 7, 1e-4)
    assert cap.iters.max() == 7 and cap.iters.min() == 2
    it, x = run_fresh(g, src, D, 7, 1e-4)
    assert np.array_equal(it, cap.iters) and err(x, cap.scores) <= TOL


# -- c. batch independence, bit for bit

def test_gpu_exact_column_does_not_depend_on_its_batch():
    """a column's summation order and its per-wave diff partials do not depend on S, so a source run
    alone equals, bit for bit, its column at position 77 of a batch of 130 after both were stopped by
    the tolerance: any leak between columns, or a stopped column that keeps changing, shows here"""
    g, src, ref = big()
    _, it, x = big_gpu()
    assert 3 < ref.iters[77] < 100
    it1, x1 = run_fresh(g, src[77:78], D, 100, 1e-4)
    assert it1[0] == it[77] == ref.iters[77]
    assert same_bits(x1[:, 0], x[:, 77])


def test_gpu_exact_rerun_on_one_handle_equals_a_fresh_handle():
    g, src, _ = small()
    ex = ppr.ExactPPR(g, src[:65], D, device=0)
    for iterations, tol in [(30, -1.0), (100, 1e-4), (7, 1e-4), (4, -1.0), (100, 1e-4)]:
        it = ex.run(iterations, tol).copy()
        x = dense(ex)
        fit, fx = run_fresh(g, src[:65], D, iterations, tol)
        assert np.array_equal(it, fit) and same_bits(x, fx), (iterations, tol)
    ex.close()


# -- d. known answers

@pytest.mark.parametrize("iterations", [1, 3, 7, 10])
def test_gpu_exact_ring_with_damping_one(iterations):
    """d = 1 on a ring: the unit mass walks one node per iteration, exactly; diff is 2 every time"""
    n = 7
    g = ppr.Csr(np.arange(n + 1), (np.arange(n) + 1) % n)
    it, x = run_fresh(g, np.arange(n), 1.0, iterations, 1e-4)
    assert (it == iterations).all()
    want = np.zeros((n, n))
    want[(np.arange(n) + iterations) % n, np.arange(n)] = 1.0
    assert same_bits(x, want)


def test_gpu_exact_damping_zero_stops_after_one():
    g, src, _ = small()
    it, x = run_fresh(g, src[:65], 0.0, 100, 1e-4)
    assert (it == 1).all()
    want = np.zeros((g.n, 65))
    want[src[:65], np.arange(65)] = 1.0
    assert same_bits(x, want)


def test_gpu_exact_dangling_source():
    """a source without successors: (1 - d) e_s after iteration 1, unchanged by iteration 2, stopped"""
    g, src, _ = small()
    s = src[np.flatnonzero(g.degrees()[src] == 0)[:2]]
    it, x = run_fresh(g, s, D, 100, 1e-4)
    assert it.tolist() == [2, 2]
    want = np.zeros((g.n, 2))
    want[s, [0, 1]] = 1.0 - D
    assert same_bits(x, want)


# -- e. gather

def test_gpu_exact_gather_of_topk_ids_is_topk_scores():
    ex, _, _ = small_gpu()
    ids, sc, ln = ex.topk(100)
    assert ln.min() == 1 and ln.max() == 100      # rows padded with -1 / 0 are part of the case
    assert same_bits(ex.gather(ids), sc)


@pytest.mark.parametrize("Q", [1, 2, 4, 197])
def test_gpu_exact_gather_shapes(Q):
    """per-row different keys, absent keys (-1, below, n and past it) among them; S * Q = 130, 260,
    520 and 25610 end in a partly filled block of 256"""
    g, src, ref = small()
    ex, _, _ = small_gpu()
    S = len(src)
    assert (S * Q) % 256 != 0
    rng = np.random.default_rng(Q)
    keys = rng.integers(-2, g.n + 3, (S, Q)).astype(np.int32)
    keys[5, 0], keys[S - 1, Q - 1] = src[5], src[S - 1]
    keys[7, 0], keys[8, Q - 1], keys[S - 2, 0] = -1, g.n, g.n + 1
    out = ex.gather(keys)
    inside = (keys >= 0) & (keys < g.n)
    assert inside.any() and (~inside).any() and out.shape == (S, Q)
    want = np.where(inside, ref.scores[np.clip(keys, 0, g.n - 1), np.arange(S)[:, None]], LD(0))
    assert np.abs(out.astype(LD) - want).max() <= TOL
    assert (out[~inside] == 0).all()
    assert out[5, 0] >= 0.15 and out[S - 1, Q - 1] >= 0.15   # a row's own source: its own column


def test_gpu_exact_gather_absent_keys():
    ex, _, _ = small_gpu()
    n, S = ex.csr.n, len(ex.sources)
    absent = np.array([-1, n, n + 1, -2 ** 31, 2 ** 31 - 1, -n], dtype=np.int32)
    assert (ex.gather(np.tile(absent, (S, 1))) == 0).all()


# -- f. top-K

def check_topk(ex, x, ref, K, tie_rows):
    """keepTop(K) of a handle whose columns are x (GPU) and ref (reference)"""
    import oracle
    ids, sc, ln = ex.topk(K)
    S = len(ex.sources)
    assert ids.shape == (S, K) and sc.shape == (S, K)
    for s in range(S):
        nz = ref.nonzero(s)
        c = min(K, len(nz))
        assert ln[s] == c, (s, ln[s], c)
        assert (ids[s, c:] == -1).all() and (sc[s, c:] == 0).all(), s
        i, v = ids[s, :c], sc[s, :c]
        assert i.min() >= 0 and i.max() < ex.csr.n and len(set(i.tolist())) == c, s
        assert ((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (i[:-1] < i[1:]))).all(), s
        top = np.sort(ref.scores[nz, s])[::-1][:c]
        assert np.abs(v.astype(LD) - top).max() <= TOL, s
        assert same_bits(v, x[i, s]), s
    for s in tie_rows:
        nz = np.flatnonzero(x[:, s] != 0)
        ki, kv = oracle.topk_row(int(ex.sources[s]), nz, x[nz, s], K)
        assert np.array_equal(ids[s, :ln[s]], ki) and same_bits(sc[s, :ln[s]], kv), s
    return ln


@pytest.mark.parametrize("K", ["1", "nz-1", "nz", "nz+1", "n+5", "100"])
def test_gpu_exact_topk_around_the_nonzero_count(K):
    """both paths of the top-K kernel at their border: everything kept (nz <= K) and the selection
    (nz > K), around source 0's nonzero count; K = 100 sorts in a row of 128"""
    g, src, ref = small()
    ex, _, x = small_gpu()
    nz = len(ref.nonzero(0))
    assert 101 < nz < g.n
    K = {"1": 1, "nz-1": nz - 1, "nz": nz, "nz+1": nz + 1, "n+5": g.n + 5, "100": 100}[K]
    ln = check_topk(ex, x, ref, K, range(len(src)))
    assert ln[0] == min(K, nz)


@pytest.mark.parametrize("K", [1, 10, 150])
def test_gpu_exact_topk_of_a_short_column(K):
    """n <= 256: the selection runs in one wave's registers"""
    g = csr(200, 7)
    src = mixed_sources(g, 12, 7)
    ref = exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 30, -1.0)
    assert max(len(ref.nonzero(s)) for s in range(12)) > 150
    ex = ppr.ExactPPR(g, src, D, device=0)
    ex.run(30, -1.0)
    x = dense(ex)
    assert err(x, ref.scores) <= TOL
    check_topk(ex, x, ref, K, range(12))
    ex.close()


def test_gpu_exact_topk_widest():
    """K = 4096, the widest row the kernels accept, out of 8200 nodes"""
    g, src, ref = big()
    ex, _, x = big_gpu()
    assert len(ref.nonzero(77)) > 4096 and len(ref.nonzero(3)) == 1
    check_topk(ex, x, ref, 4096, [77, 3, 0])


@functools.lru_cache(maxsize=None)
def layered_gpu():
    g = ppr.Csr(*graphs.layered(96, 4))
    src = np.array([0, 100, 191, 383], dtype=np.int32)
    ref = exact_ref.exact_ppr(g.row_ptr, g.col, src, D, 12, -1.0)
    ex = ppr.ExactPPR(g, src, D, device=0)
    ex.run(12, -1.0)
    return g, src, ref, ex, dense(ex)


@pytest.mark.parametrize("K", [10, 64, 100, 150, 200])
def test_gpu_exact_topk_cuts_inside_an_exact_tie(K):
    """complete layers: the nodes of a layer (but the source) share one predecessor list, so they
    carry the same score bit for bit, and every cut falls inside a tie of 95 or 96. The kept keys are
    the engine's documented tie rule (score desc, then the per-source hash of the key), restated in
    the CPU oracle, applied to the GPU's own scores."""
    g, src, ref, ex, x = layered_gpu()
    assert err(x, ref.scores) <= TOL
    for s, v in enumerate(src):
        for layer in range(4):
            nodes = np.setdiff1d(np.arange(96 * layer, 96 * layer + 96), [v])
            assert len(set(x[nodes, s].view(np.uint64).tolist())) == 1 and x[nodes[0], s] > 0, (s, layer)
    ln = check_topk(ex, x, ref, K, range(len(src)))
    assert (ln == K).all()


# -- g. benchmark_algorithm end to end

@functools.lru_cache(maxsize=None)
def harness_case():
    """a 400-node graph under shuffled string keys, the reference vectors of every node, and an
    approximate result made from them: per source the top-m keys of its reference vector with every
    9th dropped, some replaced by lower-ranked or never-reached nodes, and some scores swapped.
    m is 32, or 1, 5 or 17; a dangling source gets its own key and two nodes it never reaches (a map
    larger than its exact vector). A source enters only if every comparison the harness makes on its
    reference vector is decided by 1e-9, a thousand times the 1e-12 the GPU scores may be off."""
    n = 400
    rp, col = graphs.sparse_random(n, 21)
    rng = np.random.default_rng(21)
    name = [f"node-{p:03d}" for p in rng.permutation(n)]
    g = ppr.Csr.from_dict({name[v]: [name[u] for u in col[rp[v]:rp[v + 1]]] for v in range(n)})
    assert np.array_equal(g.row_ptr, rp) and np.array_equal(g.col, col) and g.index(name[7]) == 7
    ref = exact_ref.exact_ppr(rp, col, np.arange(n), D, 100, 1e-4)
    deg = np.diff(rp)
    res, exact, candidates = {}, {}, 0
    for v in range(n):
        x = ref.scores[:, v]
        nz = np.flatnonzero(x != 0)
        order = nz[np.lexsort((nz, -x[nz]))]
        never = np.flatnonzero(x == 0)
        if deg[v] == 0:
            if v % 2:
                continue
            keys = [v] + never[:2].tolist()
        else:
            m = {0: 1, 1: 5, 2: 17}.get(v % 10, 32)
            keys = order[:m].tolist()
            for j in range(len(keys)):
                if j % 7 == 3 and m + 2 + j < len(order):
                    keys[j] = int(order[m + 2 + j])
                elif j % 11 == 5 and len(never) > j:
                    keys[j] = int(never[j])
            keys = [k for j, k in enumerate(keys) if j % 9 != 8]
        candidates += 1
        if not exact_ref.separated(x, keys, len(keys)):
            continue
        vals = [float(x[k]) if x[k] else 1e-7 * (1 + j) for j, k in enumerate(keys)]
        for j in range(2, len(vals) - 1, 6):
            vals[j], vals[j + 1] = vals[j + 1], vals[j]
        res[name[v]] = {name[k]: s for k, s in zip(keys, vals)}
        exact[v] = x
    return g, res, exact, candidates


@pytest.mark.parametrize("strict", [True, False])
def test_gpu_benchmark_algorithm_equals_its_restatement(strict):
    g, res, exact, candidates = harness_case()
    assert len(res) >= 0.8 * candidates and candidates >= 380
    sizes = {len(m) for m in res.values()}
    dang = [k for k in res if g.degrees()[g.index(k)] == 0]
    assert {1, 3} <= sizes and len(sizes) >= 5 and len(dang) >= 3
    want = exact_ref.benchmark_ref(res, g, len(res) + 5, strict, exact)
    got = ppr.benchmark_algorithm(res, g, len(res) + 5, strict, seed=3, device=0)
    assert set(got) == set(exact_ref.FIGURES)
    for k in exact_ref.FIGURES:
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    assert 0.3 < want["jaccard average"] < 0.95 and want["kendall min"] < 0.9   # the figures discriminate


# -- h. refusals, by error code

def code_of(call):
    with pytest.raises(_lib.PprError) as e:
        call()
    return e.value.code


def test_gpu_exact_refusals():
    g, src, _ = small()
    assert code_of(lambda: ppr.ExactPPR(g, [5, -1], D, device=0)) == 12          # PPR_ERR_SOURCE
    assert code_of(lambda: ppr.ExactPPR(g, [5, g.n], D, device=0)) == 12
    assert code_of(lambda: ppr.ExactPPR(g, [], D, device=0)) == 1                # S = 0: PPR_ERR_ARG
    c = _lib.csr_struct(g.row_ptr, g.col)
    o = _lib.PprOpts(0, 0, None)
    one = np.array([5], dtype=np.int32)
    for damping in (-0.1, 1.1):
        assert code_of(lambda: ppr.ExactPPR(g, one, damping, device=0)) == 6     # PPR_ERR_DAMPING
        h = ctypes.c_void_p()                                                    # ... and by the library itself
        assert _lib.lib().ppr_exact_create(ctypes.byref(c), _lib.ptr(one), 1, damping, ctypes.byref(o),
                                           ctypes.byref(h)) == 6 and not h
    ex = ppr.ExactPPR(g, one, D, device=0)
    assert code_of(lambda: ex.run(0, 1e-4)) == 5                                 # PPR_ERR_ITERS
    ex.run(3, -1.0)
    assert code_of(lambda: ex.topk(0)) == 1                                      # PPR_ERR_ARG
    assert code_of(lambda: ex.topk(4097)) == 1
    ids, sc, ln = ex.topk(4096)                                                  # the handle still works
    assert ln[0] == len(exact_ref.exact_ppr(g.row_ptr, g.col, one, D, 3, -1.0).nonzero(0))
    ex.close()
