"""A plain high-precision restatement of the reference's exact-PPR yardstick (test helper, CPU).

  exact_ppr            pprSingleSource (include/internal/pprSingleSource.h:28-75) for S sources in
                       numpy np.longdouble (64-bit mantissa: rounding ~1e-19 per operation, seven
                       orders below the engine's 1e-12 contract), written from the recurrence:
                           x0 = e_src
                           next = (1 - d) e_src + sum over edges v -> u of x[v] * d / deg(v)
                           diff = norm1(x, next);  x = next
                       while i < iterations and diff >= tol, diff starting at tol. A dangling node
                       keeps what reaches it and passes nothing on; a repeated edge counts once per
                       repetition. A key the reference's map does not hold is a zero here.
  benchmark_ref        benchmarkAlgorithm (include/benchmarkAlgorithm.h:51-153) over those vectors:
                       keepTop(|other|), Jaccard, Kendall tau-b at the other map's keys, the five
                       figures, `strict`. Metrics are the package's jaccard / kendall_correlation,
                       pinned by tests/test_harness_host.py.
  check_rows           the golden-fixture comparison of tests/test_gpu_exact.py
  top_rows             a dense column as the recorded rows (ids, scores, counts)

Nothing here reads the HIP kernels' layout or summation order: the pull is a stable sort of the edges
by target and one np.add.reduceat.
"""
import numpy as np

LD = np.longdouble


class ExactRef:
    """scores [n, S] longdouble, iters [S] int32, diffs [T, S] longdouble (row i = the diff of
    iteration i + 1; NaN where the source had stopped before it)"""

    def __init__(self, scores, iters, diffs):
        self.scores, self.iters, self.diffs = scores, iters, diffs

    @property
    def f64(self):
        return self.scores.astype(np.float64)

    def nonzero(self, s):
        return np.flatnonzero(self.scores[:, s] != 0)


def exact_ppr(row_ptr, col, sources, damping=0.85, iterations=100, tol=1e-4):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    src = np.asarray(sources, dtype=np.int64)
    n, S = len(row_ptr) - 1, len(src)
    assert iterations > 0 and 0 <= damping <= 1 and S > 0 and src.min() >= 0 and src.max() < n
    deg = np.diff(row_ptr)
    d = LD(damping)
    fac = np.zeros(n, dtype=LD)
    fac[deg > 0] = d / deg[deg > 0].astype(LD)
    tail = np.repeat(np.arange(n, dtype=np.int64), deg)   # v of every edge v -> u
    order = np.argsort(col, kind="stable")
    tail, head = tail[order], col[order]
    if len(head):
        starts = np.flatnonzero(np.r_[True, head[1:] != head[:-1]])
        targets = head[starts]
    w = fac[tail][:, None]
    x = np.zeros((n, S), dtype=LD)
    x[src, np.arange(S)] = LD(1)
    iters = np.zeros(S, dtype=np.int32)
    diff = np.full(S, LD(tol), dtype=LD)
    diffs = []
    for _ in range(iterations):
        act = np.flatnonzero(diff >= LD(tol))
        if not len(act):
            break
        xa = x[:, act]
        nxt = np.zeros((n, len(act)), dtype=LD)
        if len(head):
            nxt[targets] = np.add.reduceat(xa[tail] * w, starts, axis=0)
        nxt[src[act], np.arange(len(act))] += LD(1) - d
        diff[act] = np.abs(nxt - xa).sum(axis=0)
        x[:, act] = nxt
        iters[act] += 1
        row = np.full(S, np.nan, dtype=LD)
        row[act] = diff[act]
        diffs.append(row)
    return ExactRef(x, iters, np.array(diffs, dtype=LD).reshape(len(diffs), S))


def top_rows(scores, K):
    """every column's nonzero entries by (score desc, id asc), cut to K: (ids [S, K] padded with -1,
    scores [S, K] padded with 0, the nonzero counts [S])"""
    n, S = scores.shape
    ids = np.full((S, K), -1, dtype=np.int32)
    sc = np.zeros((S, K), dtype=scores.dtype)
    cnt = np.zeros(S, dtype=np.int32)
    for s in range(S):
        nz = np.flatnonzero(scores[:, s] != 0)
        o = nz[np.lexsort((nz, -scores[nz, s]))][:K]
        ids[s, :len(o)], sc[s, :len(o)], cnt[s] = o, scores[o, s], len(nz)
    return ids, sc, cnt


def check_rows(ids, sc, ln, rid, rsc, rcnt, tol=1e-12):
    """rows against recorded rows: scores within tol position by position, the same keys above the
    last compared score (keys tied at the cut may fall either way)"""
    for r in range(len(ln)):
        k = min(ln[r], rcnt[r])
        assert np.abs(sc[r, :k] - rsc[r, :k]).max(initial=0.0) <= tol, r
        cut = sc[r, k - 1] if k else 0.0
        a = {i for i, s in zip(ids[r, :k], sc[r, :k]) if s > cut + tol}
        b = {i for i, s in zip(rid[r, :k], rsc[r, :k]) if s > cut + tol}
        assert a == b, r


FIGURES = ["jaccard average", "jaccard min", "kendall average", "kendall min", "average map size"]


def benchmark_ref(ppr, csr, test_nodes, strict, exact=None):
    """benchmarkAlgorithm with every eligible source sampled (test_nodes >= len(ppr), so the
    reference's shuffle picks them all and the figures do not depend on it). `exact` maps a dense
    source id to its reference column (100 iterations, 0.85, 1e-4); by default it is computed here."""
    from approximated_personalized_pagerank_amd import jaccard, kendall_correlation
    if test_nodes == 0:
        raise ValueError("testNodes must be positive")
    deg = csr.degrees()
    nodes = [k for k in ppr if not strict or deg[csr.index(k)] != 0]
    assert test_nodes >= len(nodes), "the restatement samples every source"
    if not nodes:
        return {k: -1.0 for k in FIGURES}
    if exact is None:
        src = [csr.index(k) for k in nodes]
        ref = exact_ppr(csr.row_ptr, csr.col, src, 0.85, 100, 1e-4)
        exact = {v: ref.scores[:, i] for i, v in enumerate(src)}
    js, ks, ms = [], [], []
    for k in nodes:
        other = ppr[k]
        x = exact[csr.index(k)]
        nz = np.flatnonzero(x != 0)
        top = nz[np.lexsort((nz, -x[nz]))][:len(other)]          # keepTop(|other|)
        okeys = [csr.index(o) for o in other]
        js.append(jaccard(okeys, top.tolist()))
        ks.append(kendall_correlation(list(other.values()), x[okeys].astype(np.float64)))
        ms.append(len(other))
    return {"jaccard average": float(np.mean(js)), "jaccard min": float(min(min(js), 1.0)),
            "kendall average": float(np.mean(ks)), "kendall min": float(min(min(ks), 1.0)),
            "average map size": float(np.mean(ms))}


def separated(x, okeys, m, gap=1e-9):
    """True when every comparison benchmarkAlgorithm makes on the reference column x is decided by
    more than `gap`: the nonzero values looked up at okeys pairwise, and the m-th against the
    (m + 1)-th largest at the keepTop cut"""
    v = np.sort(x[np.asarray(okeys, dtype=np.int64)])
    v = v[v != 0]
    if len(v) > 1 and np.diff(v).min() < gap:
        return False
    nzv = np.sort(x[x != 0])[::-1]
    return not (len(nzv) > m and nzv[m - 1] - nzv[m] < gap)
