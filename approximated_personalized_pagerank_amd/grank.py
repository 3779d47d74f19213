"""Python mirror of the reference's GRank surface, running on the MI355X HIP engine.

    grank(graph, K, L, iterations, damping, tolerance)                 include/grank.h:42-48
    grank_multi(graph, K, L, iterations, damping, tolerance, nThreads) header-only/grankMulti.h:289-296

Same argument meaning, same validation messages (raised as PprError instead of the reference's
``cerr`` + ``exit(EXIT_FAILURE)``), same result shape: {source: {node: score}} with at most K
entries per source. Ties at the top-L / top-K cut are broken by (score desc, dense id asc);
the reference leaves them to unordered_map order (DESIGN.md "parity contract").
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Hashable, Optional, Sequence

import numpy as np

from . import _lib
from .graph import Csr


def _check_params(K, L, iterations, damping):
    # include/grank.h:51-55 (in this order)
    if K == 0:
        raise _lib.PprError(2)
    if L == 0:
        raise _lib.PprError(3)
    if K > L:
        raise _lib.PprError(4)
    if iterations == 0:
        raise _lib.PprError(5)
    if damping < 0 or damping > 1:
        raise _lib.PprError(6)
    if K < 0 or L < 0 or iterations < 0:
        raise _lib.PprError(1)


@dataclass
class GrankResult:
    ids: np.ndarray        # int32 [n, K] dense ids, score desc / id asc, -1 padded
    scores: np.ndarray     # float64 [n, K]
    lens: np.ndarray       # int32 [n]
    iterations_run: int = 0
    max_diff: Optional[np.ndarray] = None
    device_ms: float = 0.0
    merge_ms: float = 0.0
    candidates: int = 0
    algo_bytes: int = 0

    def to_dict(self, csr: Csr) -> Dict[Hashable, Dict[Hashable, float]]:
        out = {}
        for v in range(csr.n):
            k = int(self.lens[v])
            out[csr.key(v)] = {csr.key(int(i)): float(s) for i, s in zip(self.ids[v, :k], self.scores[v, :k])}
        return out


@dataclass
class QueryResult:
    """Answer of GrankPlan.query: row q = the K best (id, score) of query q's preference set."""
    ids: np.ndarray        # int32 [Q, K] dense ids, score desc / id asc, -1 padded
    scores: np.ndarray     # float64 [Q, K]
    lens: np.ndarray       # int32 [Q]
    device_ms: float = 0.0
    candidates: int = 0
    algo_bytes: int = 0
    wave_queries: int = 0
    wg_queries: int = 0
    range_queries: int = 0
    max_ranges: int = 0

    def to_dicts(self, csr: Csr):
        """one {graph key: score} per query, like GrankResult.to_dict's rows"""
        return [{csr.key(int(i)): float(s) for i, s in zip(self.ids[q, :int(k)], self.scores[q, :int(k)])}
                for q, k in enumerate(self.lens)]


@dataclass
class RQueryResult:
    """Answer of GrankPlan.rquery: row q = the K best (source, score) for query q's target set."""
    ids: np.ndarray        # int32 [Q, K] dense source ids, score desc / id asc, -1 padded
    scores: np.ndarray     # float64 [Q, K]
    lens: np.ndarray       # int32 [Q]
    device_ms: float = 0.0
    hits: int = 0
    algo_bytes: int = 0
    probe_queries: int = 0
    scan_queries: int = 0
    scans: int = 0
    chunks: int = 0

    def to_dicts(self, csr: Csr):
        """one {graph key of the source: score} per query"""
        return [{csr.key(int(i)): float(s) for i, s in zip(self.ids[q, :int(k)], self.scores[q, :int(k)])}
                for q, k in enumerate(self.lens)]


@dataclass
class SweepResult:
    """Answer of GrankPlan.sweep / sweep_vectors: row i = the sweep of source (or vector) i and its
    prefix of lowest conductance."""
    order: np.ndarray      # int32 [S, width] the swept members in sweep order, -1 padded
    swept: np.ndarray      # int32 [S] members swept (before max_size and the volume cap stopped it)
    size: np.ndarray       # int32 [S] members of the best prefix, 0: none admissible
    cut: np.ndarray        # int64 [S] edges leaving it
    vol: np.ndarray        # int64 [S] its volume
    phi: np.ndarray        # float64 [S] cut / min(vol, m - vol), +inf with size 0
    profile_cut: Optional[np.ndarray] = None   # int64 [S, width] cut_j at j - 1, -1 padded (profile=True)
    profile_vol: Optional[np.ndarray] = None   # int64 [S, width] vol_j at j - 1

    def sets(self):
        """the best set of each row: int32 arrays of dense ids, in sweep order"""
        return [self.order[i, :int(k)].copy() for i, k in enumerate(self.size)]

    def to_dicts(self, csr: Csr):
        """one {graph key: rank in the sweep} per row, the best sets keyed by the graph's own keys"""
        return [{csr.key(int(v)): j for j, v in enumerate(self.order[i, :int(k)])} for i, k in enumerate(self.size)]


@dataclass
class SubgraphBatch:
    """Answer of GrankPlan.subgraphs: the subgraphs induced by each source's top PPR neighbours, as one
    batched graph. Tensors live on the plan's device; member j of position i has the batch id
    node_ptr[i] + j, and the edges of position i are edge_ptr[i] .. edge_ptr[i + 1] - 1."""
    nodes: "torch.Tensor"            # [N] dense ids of the members, position by position, in rank order
    scores: "Optional[torch.Tensor]"  # [N] float64, the row's score of each member (scores=True)
    rowptr: "torch.Tensor"           # [N + 1] CSR over batch ids
    col: "torch.Tensor"              # [E] batch id of every edge's target
    row: "Optional[torch.Tensor]"    # [E] batch id of every edge's source (coo=True)
    eid: "Optional[torch.Tensor]"    # [E] int64, the edge's position in the plan's edge array (edge_ids=True)
    node_ptr: np.ndarray             # int64 [S + 1]
    edge_ptr: np.ndarray             # int64 [S + 1]

    @property
    def num_graphs(self) -> int:
        return len(self.node_ptr) - 1

    @property
    def num_nodes(self) -> int:
        return int(self.node_ptr[-1])

    @property
    def num_edges(self) -> int:
        return int(self.edge_ptr[-1])

    @property
    def edge_index(self):
        """[2, E]: row over col, the COO form message-passing layers take (needs coo=True)"""
        import torch
        if self.row is None:
            raise ValueError("edge_index needs the COO rows: call subgraphs(coo=True)")
        return torch.stack((self.row, self.col))

    @property
    def roots(self):
        """[S] int64, the batch id of member 0 of every position (the source itself with root_first=True)"""
        import torch
        return torch.as_tensor(self.node_ptr[:-1].copy(), dtype=torch.int64, device=self.nodes.device)

    @property
    def batch(self):
        """[N] int64, the position every node belongs to"""
        import torch
        counts = torch.as_tensor(np.diff(self.node_ptr), dtype=torch.int64, device=self.nodes.device)
        return torch.repeat_interleave(torch.arange(self.num_graphs, dtype=torch.int64, device=self.nodes.device), counts)


PAIR_OUTPUTS = ("fwd", "bwd", "rank", "common", "dot")


@dataclass
class PairResult:
    """Answer of GrankPlan.pairs / pair_scores: one entry per (source, candidate) pair, in candidate
    order; group q = pairs gptr[q] .. gptr[q + 1] - 1, all scored against sources[q]. The arrays of
    outputs that were not asked for are None."""
    sources: np.ndarray              # int32 [Q]
    candidates: np.ndarray           # int32 [P]
    gptr: np.ndarray                 # int64 [Q + 1]
    hit: np.ndarray                  # uint8 [P] bit 0: v is a key of B[u]; bit 1: u is a key of B[v]
    src_len: np.ndarray              # int32 [Q] entries of B[u]
    cand_len: np.ndarray             # int32 [P] entries of B[v]
    fwd: Optional[np.ndarray] = None     # float64 [P] B[u][v], 0 when absent
    bwd: Optional[np.ndarray] = None     # float64 [P] B[v][u], 0 when absent
    rank: Optional[np.ndarray] = None    # int32 [P] position of v in B[u] by (score desc, id asc), -1 when absent
    common: Optional[np.ndarray] = None  # int32 [P] keys the two rows share
    dot: Optional[np.ndarray] = None     # float64 [P] exact dot product of the two rows, rounded once

    @property
    def pair_sources(self) -> np.ndarray:
        """int32 [P]: the source of every pair"""
        return np.repeat(self.sources, np.diff(self.gptr))

    @property
    def pair_src_len(self) -> np.ndarray:
        """int32 [P]: len(B[u]) of every pair"""
        return np.repeat(self.src_len, np.diff(self.gptr))

    def jaccard(self) -> np.ndarray:
        """common / (len_u + len_v - common) per pair, 0 where the denominator is 0 (needs "common")"""
        if self.common is None:
            raise ValueError('jaccard needs the overlap: ask for what=("common", ...)')
        c = self.common.astype(np.float64)
        den = self.pair_src_len.astype(np.float64) + self.cand_len.astype(np.float64) - c
        return np.divide(c, den, out=np.zeros(len(c), dtype=np.float64), where=den > 0)

    def cosine(self, norm2_u, norm2_v) -> np.ndarray:
        """dot / sqrt(norm2_u * norm2_v) per pair, 0 where a norm is 0 (needs "dot"). norm2_u: the squared
        norm of every group's source row (length Q) or of every pair's (length P); norm2_v: of every
        pair's candidate row. The squared norm of row x is dot(x, x): plan.pair_scores(x, x, what=("dot",)).dot"""
        if self.dot is None:
            raise ValueError('cosine needs the dot products: ask for what=("dot", ...)')
        nu = np.asarray(norm2_u, dtype=np.float64).reshape(-1)
        nv = np.asarray(norm2_v, dtype=np.float64).reshape(-1)
        P = len(self.candidates)
        if len(nu) == len(self.sources) and len(nu) != P:
            nu = np.repeat(nu, np.diff(self.gptr))
        if len(nu) != P or len(nv) != P:
            raise ValueError(f"norms: {len(nu)} and {len(nv)} values for {len(self.sources)} groups and {P} pairs")
        den = np.sqrt(nu * nv)
        return np.divide(self.dot, den, out=np.zeros(P, dtype=np.float64), where=den > 0)

    def to_dicts(self, csr: Csr):
        """one {graph key of the candidate: {output: value}} per group, keyed by the graph's own keys (a
        candidate repeated within a group keeps its last entry)"""
        names = [f for f in ("fwd", "bwd", "rank", "common", "dot") if getattr(self, f) is not None]
        out = []
        for q in range(len(self.sources)):
            d = {}
            for j in range(int(self.gptr[q]), int(self.gptr[q + 1])):
                e = {f: getattr(self, f)[j].item() for f in names}
                e["hit"] = int(self.hit[j])
                d[csr.key(int(self.candidates[j]))] = e
            out.append(d)
        return out


def _int32_ids(x, what):
    flat = np.asarray(x, dtype=np.int64).reshape(-1)
    if len(flat) and (flat.min() < -2**31 or flat.max() >= 2**31):
        raise ValueError(f"{what} ids must fit in int32")
    return np.ascontiguousarray(flat, dtype=np.int32)


def normalize_groups(sources, candidates):
    """The CSR form ppr_grank_plan_pairs takes: (gptr int64 [Q+1], sources int32 [Q], cands int32 [P]).
    `candidates` is (gptr, cands) arrays or a sequence of candidate sequences, one per source. Shape
    mismatches raise ValueError."""
    src = _int32_ids(sources, "source")
    gptr, cands, _ = normalize_queries(candidates)
    if len(gptr) - 1 != len(src):
        raise ValueError(f"candidates: {len(gptr) - 1} groups for {len(src)} sources")
    return gptr, src, cands


def normalize_pairs(u, v):
    """Flat pairs (u[i], v[i]) grouped by source for ppr_grank_plan_pairs: returns (gptr, sources,
    cands, order, inverse). The pairs are sorted by u with a stable sort (`order`: pair order[j] of the
    caller stands at position j, so equal sources keep the caller's order of candidates); sources are the
    distinct values of u ascending; `inverse` scatters back: result_in_caller_order = result[inverse].
    Arrays of different lengths or more than one dimension raise ValueError."""
    ua, va = np.asarray(u), np.asarray(v)
    if ua.ndim != 1 or va.ndim != 1:
        raise ValueError(f"u and v must be flat arrays, not {ua.ndim}-D and {va.ndim}-D")
    if len(ua) != len(va):
        raise ValueError(f"u has {len(ua)} entries, v {len(va)}")
    ua, va = _int32_ids(ua, "source"), _int32_ids(va, "candidate")
    order = np.argsort(ua, kind="stable")
    su = ua[order]
    if len(su):
        first = np.flatnonzero(np.concatenate(([True], su[1:] != su[:-1])))
        sources = su[first]
        gptr = np.concatenate((first, [len(su)])).astype(np.int64)
    else:
        sources, gptr = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
    inverse = np.empty(len(order), dtype=np.int64)
    inverse[order] = np.arange(len(order), dtype=np.int64)
    return gptr, np.ascontiguousarray(sources), np.ascontiguousarray(va[order]), order, inverse


def pair_outputs(what):
    """the outputs named in `what`, validated: a tuple in PAIR_OUTPUTS order"""
    if isinstance(what, str):
        what = (what,)
    what = tuple(what)
    bad = [w for w in what if w not in PAIR_OUTPUTS]
    if bad or not what:
        raise ValueError(f"what must name some of {PAIR_OUTPUTS}, not {what!r}")
    return tuple(w for w in PAIR_OUTPUTS if w in what)


def subgraph_arguments(size, max_deg, edge_capacity=None):
    """(size, max_deg, edge_capacity) as the C call takes them (None: 0, the library's default; no
    capacity: None); a value its words cannot carry is refused here, as PprError(invalid argument),
    a size the library would refuse as PprError(out of range)"""
    sz, md = 0 if size is None else int(size), 0 if max_deg is None else int(max_deg)
    cap = None if edge_capacity is None else int(edge_capacity)
    if not (0 <= sz < 2**32) or not (0 <= md < 2**63) or (cap is not None and not (0 <= cap < 2**63)):
        raise _lib.PprError(1, "plan_subgraphs")
    if (size is not None and sz == 0) or (max_deg is not None and md == 0):  # (0 means "none" only as the default)
        raise _lib.PprError(1, "plan_subgraphs")
    if sz > 4096:  # (no tensor is allocated for a call the library refuses)
        raise _lib.PprError(11, "plan_subgraphs")
    return sz, md, cap


def normalize_queries(queries, weights=None):
    """The CSR form ppr_grank_plan_query takes: (qptr int64 [Q+1], seeds int32, weights float64 or
    None). `queries` is (qptr, seeds) arrays or a sequence of seed sequences; `weights` a flat array
    or a sequence of sequences of the same shape. Shape mismatches raise ValueError."""
    is_csr = (isinstance(queries, tuple) and len(queries) == 2 and isinstance(queries[0], np.ndarray)
              and isinstance(queries[1], np.ndarray))
    if is_csr:
        qptr = np.ascontiguousarray(queries[0], dtype=np.int64)
        seeds = np.ascontiguousarray(queries[1], dtype=np.int32)
        if qptr.ndim != 1 or seeds.ndim != 1 or len(qptr) < 1 or qptr[0] != 0 or qptr[-1] != len(seeds):
            raise ValueError("queries=(qptr, seeds): qptr must start at 0 and end at len(seeds)")
        if np.any(np.diff(qptr) < 0):
            raise ValueError("queries=(qptr, seeds): qptr must not decrease")
    else:
        rows = [np.asarray(q, dtype=np.int64).reshape(-1) for q in queries]
        qptr = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            np.cumsum([len(r) for r in rows], out=qptr[1:])
        flat = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        if len(flat) and (flat.min() < -2**31 or flat.max() >= 2**31):
            raise ValueError("seed ids must fit in int32")
        seeds = np.ascontiguousarray(flat, dtype=np.int32)
    if weights is None:
        return qptr, seeds, None
    flat_w = (isinstance(weights, np.ndarray) and weights.ndim == 1 and weights.dtype != object) or (
        not isinstance(weights, np.ndarray) and len(weights) > 0 and all(np.isscalar(x) for x in weights))
    if flat_w:
        w = np.ascontiguousarray(weights, dtype=np.float64)
    else:
        wrows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in weights]
        if len(wrows) != len(qptr) - 1:
            raise ValueError(f"weights: {len(wrows)} rows for {len(qptr) - 1} queries")
        for q, r in enumerate(wrows):
            if len(r) != qptr[q + 1] - qptr[q]:
                raise ValueError(f"weights: row {q} has {len(r)} entries for {qptr[q + 1] - qptr[q]} seeds")
        w = np.ascontiguousarray(np.concatenate(wrows) if wrows else np.zeros(0), dtype=np.float64)
    if len(w) != len(seeds):
        raise ValueError(f"weights: {len(w)} entries for {len(seeds)} seeds")
    return qptr, seeds, w


def normalize_vectors(ids_or_result, scores=None, lens=None):
    """The rows ppr_grank_plan_sweep_vectors takes: (ids int32 [R, W], scores float64 [R, W], lens
    int32 [R]). `ids_or_result` is a QueryResult (or any object with .ids / .scores / .lens) or an id
    array, then with `scores`; `lens` None: a row ends at its first id -1. Shape mismatches raise
    ValueError."""
    if scores is None and all(hasattr(ids_or_result, f) for f in ("ids", "scores", "lens")):
        if lens is not None:
            raise ValueError("lens given with a result object that has its own")
        ids_or_result, scores, lens = ids_or_result.ids, ids_or_result.scores, ids_or_result.lens
    if scores is None:
        raise ValueError("scores are required with an id array")
    raw = np.asarray(ids_or_result)
    if raw.ndim != 2:
        raise ValueError(f"ids must be 2-D [rows, width], not {raw.ndim}-D")
    if raw.size and (raw.min() < -2**31 or raw.max() >= 2**31):
        raise ValueError("ids must fit in int32")
    ids = np.ascontiguousarray(raw, dtype=np.int32)
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    if sc.shape != ids.shape:
        raise ValueError(f"scores have shape {sc.shape}, ids {ids.shape}")
    if lens is None:
        ln = np.where((ids < 0).any(axis=1), (ids < 0).argmax(axis=1), ids.shape[1]).astype(np.int32)
    else:
        ln = np.ascontiguousarray(np.asarray(lens).reshape(-1), dtype=np.int32)
        if len(ln) != ids.shape[0]:
            raise ValueError(f"lens: {len(ln)} entries for {ids.shape[0]} rows")
    return ids, sc, ln


def sweep_arguments(min_size, max_size, max_vol):
    """(min_size, max_size, max_vol) as the C call takes them (None: 0, the library's default); a value
    that its unsigned / signed words cannot carry is refused here, as PprError(invalid argument)"""
    mn, mx, mv = int(min_size), 0 if max_size is None else int(max_size), 0 if max_vol is None else int(max_vol)
    if not (0 <= mn < 2**32) or not (0 <= mx < 2**32) or not (-2**63 <= mv < 2**63):
        raise _lib.PprError(1, "plan_sweep")
    if max_size is not None and mx == 0:  # (0 means "the row width" only as the default)
        raise _lib.PprError(1, "plan_sweep")
    return mn, mx, mv


def _stats_to(res: GrankResult, st: _lib.PprStats) -> None:
    res.iterations_run = int(st.iterations_run)
    res.max_diff = np.array(st.max_diff[: min(st.iterations_run, _lib.PPR_MAX_ITER_STATS)])
    res.device_ms = float(st.device_ms)
    res.merge_ms = float(st.merge_ms)
    res.candidates = int(st.candidates)
    res.algo_bytes = int(st.algo_bytes)


def _flags(stats: bool, sum_mode: Optional[str]) -> int:
    """sum_mode: None = the library default (exact, or PPR_SUM), "exact", or "chain" (the
    reference's in-order fma sums, include/grank.h:107-116)"""
    if sum_mode not in (None, "exact", "chain"):
        raise ValueError(f"sum_mode must be 'exact' or 'chain', not {sum_mode!r}")
    return (_lib.PPR_FLAG_STATS if stats else 0) | (_lib.PPR_FLAG_CHAIN_SUM if sum_mode == "chain" else 0)


def grank_csr(csr: Csr, K: int, L: int, iterations: int, damping: float, tolerance: float,
              part: Optional[np.ndarray] = None, device: int = -1, stats: bool = False,
              sum_mode: Optional[str] = None) -> GrankResult:
    """GRank over a dense CSR graph on one MI355X (synchronous)."""
    _check_params(K, L, iterations, damping)
    n = csr.n
    ids = np.full((n, K), -1, dtype=np.int32)
    sc = np.zeros((n, K), dtype=np.float64)
    lens = np.zeros(n, dtype=np.int32)
    res = GrankResult(ids, sc, lens)
    if n == 0:
        return res
    # part="plan": none given -- plan creation computes them (on the device, the host BFS as fallback),
    # as for the C++ drop-in templates
    if isinstance(part, str) and part == "plan":
        p = None
    else:
        p = csr.partitions() if part is None else np.ascontiguousarray(part, dtype=np.uint8)
    c = _lib.csr_struct(csr.row_ptr, csr.col)
    o = _lib.PprOpts(device, _flags(stats, sum_mode), None)
    st = _lib.PprStats()
    rc = _lib.lib().ppr_grank_csr(ctypes.byref(c), _lib.ptr(p), K, L, iterations, damping, tolerance,
                                  ctypes.byref(o), _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(lens),
                                  ctypes.byref(st))
    _lib.check(rc, "ppr_grank_csr")
    _stats_to(res, st)
    return res


def grank(graph: Dict[Hashable, Sequence[Hashable]], K: int, L: int, iterations: int, damping: float,
          tolerance: float) -> Dict[Hashable, Dict[Hashable, float]]:
    """ppr::grank (include/grank.h:42-150) on the GPU."""
    _check_params(K, L, iterations, damping)
    csr = Csr.from_dict(graph)
    return grank_csr(csr, K, L, iterations, damping, tolerance).to_dict(csr)


def grank_multi(graph: Dict[Hashable, Sequence[Hashable]], K: int, L: int, iterations: int,
                damping: float, tolerance: float, nThreads: int) -> Dict[Hashable, Dict[Hashable, float]]:
    """ppr::grankMulti (header-only/grankMulti.h:289-436): identical output to grank; the
    thread count only sizes host-side work (the merge runs on the GPU)."""
    _check_params(K, L, iterations, damping)
    if nThreads == 0:
        raise _lib.PprError(7)
    return grank(graph, K, L, iterations, damping, tolerance)


class GrankPlan:
    """Device-resident GRank plan (inputs uploaded once; run() is the device phase only)."""

    def __init__(self, csr: Csr, K: int, L: int, damping: float, part: Optional[np.ndarray] = None,
                 device: int = -1, stream: Optional[int] = None, stats: bool = False,
                 sum_mode: Optional[str] = None):
        _check_params(K, L, 1, damping)
        self.csr, self.K, self.L = csr, K, L
        self._p = ctypes.c_void_p()
        p = csr.partitions() if part is None else np.ascontiguousarray(part, dtype=np.uint8)
        self.part = p
        c = _lib.csr_struct(csr.row_ptr, csr.col)
        o = _lib.PprOpts(device, _flags(stats, sum_mode), stream)
        _lib.check(_lib.lib().ppr_grank_plan_create(ctypes.byref(c), _lib.ptr(p), K, L, damping,
                                                    ctypes.byref(o), ctypes.byref(self._p)), "plan_create")
        self.iterations_run = 0

    def close(self):
        if self._p:
            _lib.lib().ppr_grank_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return _lib.lib().ppr_grank_plan_stream(self._p) or 0

    def run(self, iterations: int, tolerance: float) -> _lib.PprStats:
        st = _lib.PprStats()
        _lib.check(_lib.lib().ppr_grank_plan_run(self._p, iterations, tolerance, ctypes.byref(st)), "plan_run")
        self.iterations_run = int(st.iterations_run)
        return st

    KERNEL_GROUPS = ("wave tier k_merge_lds_x", "sieve large k_sv1+k_svfin (16 waves)",
                     "sieve mid k_sv1+k_svfin (8 waves)", "sieve small k_sv1+k_svfin (4 waves)",
                     "sieve multi-slice k_svA+k_svB+k_svF", "range k_xr+k_xfinal+k_xfin1")

    def kernel_stats(self):
        """per kernel group of the last run(): SURVEY s8d algorithmic bytes of the sources it merged,
        HIP event milliseconds on its stream, event pairs (include/ppr_hip.h ppr_grank_plan_kernel_stats)"""
        n = len(self.KERNEL_GROUPS)
        b = np.zeros(n)
        ms = np.zeros(n)
        la = np.zeros(n, dtype=np.int64)
        _lib.check(_lib.lib().ppr_grank_plan_kernel_stats(self._p, n, _lib.ptr(b), _lib.ptr(ms), _lib.ptr(la)),
                   "kernel_stats")
        return {name: {"algo_bytes": float(b[i]), "ms": float(ms[i]), "launches": int(la[i])}
                for i, name in enumerate(self.KERNEL_GROUPS)}

    # step-level API (source sharding)
    def init(self):
        _lib.check(_lib.lib().ppr_grank_plan_init(self._p), "plan_init")

    def active_count(self, it: int) -> int:
        c = ctypes.c_int64()
        _lib.check(_lib.lib().ppr_grank_plan_active_count(self._p, it, ctypes.byref(c)), "active_count")
        return int(c.value)

    def iterate(self, it: int, begin: int, end: int):
        _lib.check(_lib.lib().ppr_grank_plan_iterate(self._p, it, begin, end), "plan_iterate")

    def read_maxdiff(self, it: int) -> float:
        d = ctypes.c_double()
        _lib.check(_lib.lib().ppr_grank_plan_read_maxdiff(self._p, it, ctypes.byref(d)), "read_maxdiff")
        return float(d.value)

    def finish(self, iterations_run: int):
        self.iterations_run = iterations_run
        _lib.check(_lib.lib().ppr_grank_plan_finish(self._p, iterations_run), "plan_finish")

    def fetch(self) -> GrankResult:
        n, K = self.csr.n, self.K
        ids = np.full((n, K), -1, dtype=np.int32)
        sc = np.zeros((n, K), dtype=np.float64)
        lens = np.zeros(n, dtype=np.int32)
        _lib.check(_lib.lib().ppr_grank_plan_fetch(self._p, _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(lens)), "fetch")
        return GrankResult(ids, sc, lens, self.iterations_run)

    def fetch_slab(self, iterations_run: Optional[int] = None):
        it = self.iterations_run if iterations_run is None else iterations_run
        n, L = self.csr.n, self.L
        ids = np.full((n, L), -1, dtype=np.int32)
        sc = np.zeros((n, L), dtype=np.float64)
        lens = np.zeros(n, dtype=np.int32)
        _lib.check(_lib.lib().ppr_grank_plan_fetch_slab(self._p, it, _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(lens)),
                   "fetch_slab")
        return ids, sc, lens

    def _resident_query(self, symbol, where, queries, K, weights, flags, iterations_run, st, counters):
        """the call both query directions make: (ids, scores, lens, device_ms, *the stats' integer counters)"""
        qptr, ids_in, w = normalize_queries(queries, weights)
        Q = len(qptr) - 1
        it = self.iterations_run if iterations_run is None else iterations_run
        ids = np.full((Q, max(K, 0)), -1, dtype=np.int32)
        sc = np.zeros((Q, max(K, 0)), dtype=np.float64)
        lens = np.zeros(Q, dtype=np.int32)
        if K < 0 or K >= 2**32:
            raise _lib.PprError(1, where)
        _lib.check(getattr(_lib.lib(), symbol)(self._p, it, Q, _lib.ptr(qptr), _lib.ptr(ids_in), _lib.ptr(w), K, flags,
                                               _lib.ptr(ids), _lib.ptr(sc), _lib.ptr(lens), ctypes.byref(st)), where)
        return (ids, sc, lens, float(st.device_ms)) + tuple(int(getattr(st, f)) for f in counters)

    def query(self, queries, K: int, weights=None, exclude_seeds: bool = False,
              iterations_run: Optional[int] = None) -> QueryResult:
        """PageRank personalised to each query's seed set, from the plan's resident baskets
        (include/ppr_hip.h ppr_grank_plan_query): by linearity the weighted sum of the seeds' own
        vectors, summed exactly, the K best by (score desc, dense id asc). `queries`: (qptr, seeds)
        arrays or a sequence of seed sequences of dense ids; `weights`: None (all 1), a flat array
        or sequences of the same shape; `iterations_run` defaults to the plan's last run."""
        return QueryResult(*self._resident_query("ppr_grank_plan_query", "plan_query", queries, K, weights,
                                                 _lib.PPR_QUERY_EXCLUDE_SEEDS if exclude_seeds else 0, iterations_run,
                                                 _lib.PprQueryStats(), ("candidates", "algo_bytes", "wave_queries",
                                                                        "wg_queries", "range_queries", "max_ranges")))

    def rquery(self, queries, K: int, weights=None, exclude_targets: bool = False,
               iterations_run: Optional[int] = None) -> RQueryResult:
        """The sources that rank each query's weighted target set highest, from the plan's resident
        baskets (include/ppr_hip.h ppr_grank_plan_rquery): score(u) = sum_j f_j B[u][t_j] over the
        targets that are keys of u's basket, summed exactly, the K best sources by (score desc,
        dense id asc). Arguments as for query(); `exclude_targets` drops the sources that are
        targets of their query."""
        return RQueryResult(*self._resident_query("ppr_grank_plan_rquery", "plan_rquery", queries, K, weights,
                                                  _lib.PPR_RQUERY_EXCLUDE_TARGETS if exclude_targets else 0,
                                                  iterations_run, _lib.PprRQueryStats(),
                                                  ("hits", "algo_bytes", "probe_queries", "scan_queries", "scans",
                                                   "chunks")))

    # ---- sweep cuts (include/ppr_hip.h ppr_grank_plan_sweep / _sweep_vectors) ----
    def _sweep(self, where, rows, row_width, call, min_size, max_size, max_vol, profile, stats):
        mn, mx, mv = sweep_arguments(min_size, max_size, max_vol)
        width = max(0, (min(mx, row_width) if where == "plan_sweep_vectors" else mx) if mx else row_width)
        if mx > 4096:  # (no array of that width is allocated for a call the library refuses)
            raise _lib.PprError(11, where)
        order = np.full((rows, width), -1, dtype=np.int32)
        swept = np.zeros(rows, dtype=np.int32)
        size = np.zeros(rows, dtype=np.int32)
        cut = np.zeros(rows, dtype=np.int64)
        vol = np.zeros(rows, dtype=np.int64)
        phi = np.full(rows, np.inf, dtype=np.float64)
        pc = np.full((rows, width), -1, dtype=np.int64) if profile else None
        pv = np.full((rows, width), -1, dtype=np.int64) if profile else None
        st = _lib.PprSweepStats()
        _lib.check(call(mn, mx, mv, 0, _lib.ptr(order), _lib.ptr(swept), _lib.ptr(size), _lib.ptr(cut), _lib.ptr(vol),
                        _lib.ptr(phi), _lib.ptr(pc), _lib.ptr(pv), ctypes.byref(st)), where)
        if stats is not None:
            stats.update(device_ms=float(st.device_ms), edges=int(st.edges), algo_bytes=int(st.algo_bytes),
                         wave_sources=int(st.wave_sources), wg_sources=int(st.wg_sources),
                         slice_sources=int(st.slice_sources), chunks=int(st.chunks))
        return SweepResult(order, swept, size, cut, vol, phi, pc, pv)

    def sweep(self, sources=None, min_size: int = 1, max_size: Optional[int] = None, max_vol: Optional[int] = None,
              profile: bool = False, iterations_run: Optional[int] = None, stats: Optional[dict] = None) -> SweepResult:
        """The sweep cut of each source's resident PPR row, on the device (include/ppr_hip.h
        ppr_grank_plan_sweep): the row ordered by score / out-degree, cut at `max_size` entries (None:
        the row width L) and before the volume exceeds `max_vol` (None: half the graph's edges), and
        the prefix of at least `min_size` members with the lowest conductance. sources: dense ids
        (None: every node, in order); profile: also the cut and the volume of every prefix; stats: a
        dict that receives the call's ppr_sweep_stats. The graph is taken as directed; pass a
        symmetric graph for undirected clustering."""
        S, src = self._prop_sources(sources)
        it = self.iterations_run if iterations_run is None else iterations_run
        fn = _lib.lib().ppr_grank_plan_sweep
        if src is not None and S == 0:  # (an empty list is not "every node": the pointer must not be null)
            src = np.zeros(1, dtype=np.int32)
        return self._sweep("plan_sweep", S, self.L, lambda *tail: fn(self._p, it, S, _lib.ptr(src), *tail), min_size,
                           max_size, max_vol, profile, stats)

    def sweep_vectors(self, ids_or_result, scores=None, lens=None, min_size: int = 1, max_size: Optional[int] = None,
                      max_vol: Optional[int] = None, profile: bool = False, stats: Optional[dict] = None) -> SweepResult:
        """The same sweep over caller-supplied sparse vectors on the plan's graph (include/ppr_hip.h
        ppr_grank_plan_sweep_vectors): a QueryResult (the community of a seed set), an exact PPR
        top-K, or any (ids [R, W], scores [R, W], lens [R]) with W <= 4096 and distinct ids per row."""
        ids, sc, ln = normalize_vectors(ids_or_result, scores, lens)
        R, W = ids.shape
        fn = _lib.lib().ppr_grank_plan_sweep_vectors
        # a pointer for empty rows too: the C call refuses null pointers, and reads nothing through it
        dummy = np.zeros(1, dtype=np.float64)
        pi, ps = (_lib.ptr(ids), _lib.ptr(sc)) if ids.size else (_lib.ptr(dummy), _lib.ptr(dummy))
        pl = _lib.ptr(ln) if len(ln) else _lib.ptr(dummy)
        return self._sweep("plan_sweep_vectors", R, W, lambda *tail: fn(self._p, R, W, pi, ps, pl, *tail), min_size,
                           max_size, max_vol, profile, stats)

    # ---- induced subgraph batches (include/ppr_hip.h ppr_grank_plan_subgraphs) ----
    def subgraphs(self, sources=None, size: Optional[int] = None, max_deg: Optional[int] = None, root_first: bool = False,
                  index_dtype=None, coo: bool = True, edge_ids: bool = False, scores: bool = True,
                  iterations_run: Optional[int] = None, edge_capacity: Optional[int] = None,
                  stats: Optional[dict] = None) -> SubgraphBatch:
        """The subgraph each source's top PPR neighbours induce, for a whole minibatch, on the device
        (include/ppr_hip.h ppr_grank_plan_subgraphs): the `size` best entries of the source's resident
        row (None: the row width L) by (score desc, id asc), the source first with `root_first`, and
        every stored edge between them (members of more than `max_deg` out-edges emit none). Returns
        a SubgraphBatch of torch tensors on the plan's device: `index_dtype` torch.int64 (default) or
        torch.int32; coo: also the COO rows; edge_ids: also every edge's position in the graph's edge
        array; scores: also the members' scores. By default a count-only call sizes the tensors exactly;
        `edge_capacity` skips it (a guess that is too small costs one more call). sources: dense ids
        (None: every node, in order); stats: a dict that receives the call's ppr_subg_stats."""
        import torch
        if index_dtype is None:
            index_dtype = torch.int64
        if index_dtype not in (torch.int32, torch.int64):
            raise TypeError(f"index_dtype must be torch.int32 or torch.int64, not {index_dtype}")
        sz, md, cap = subgraph_arguments(size, max_deg, edge_capacity)
        S, src = self._prop_sources(sources)
        if src is not None and S == 0:  # (an empty list is not "every node": the pointer must not be null)
            src = np.zeros(1, dtype=np.int32)
        it = self.iterations_run if iterations_run is None else iterations_run
        flags = (_lib.PPR_SUBG_ROOT_FIRST if root_first else 0) | (_lib.PPR_SUBG_IDX64 if index_dtype == torch.int64 else 0)
        node_ptr = np.zeros(S + 1, dtype=np.int64)
        edge_ptr = np.zeros(S + 1, dtype=np.int64)
        st = _lib.PprSubgStats()
        fn = _lib.lib().ppr_grank_plan_subgraphs
        dev = torch.device("cuda", self.device)

        def call(ncap, ecap, t):
            return fn(self._p, it, S, _lib.ptr(src), sz, md, flags, ncap, ecap, _lib.ptr(node_ptr), _lib.ptr(edge_ptr),
                      *(None if x is None else x.data_ptr() for x in t), ctypes.byref(st))

        def alloc(ncap, ecap):
            # (one spare element each: data_ptr() of an empty tensor is null, and a null pointer means count-only)
            t = (torch.empty(ncap + 1, dtype=index_dtype, device=dev),
                 torch.empty(ncap + 1, dtype=torch.float64, device=dev) if scores else None,
                 torch.empty(ncap + 1, dtype=index_dtype, device=dev),
                 torch.empty(ecap + 1, dtype=index_dtype, device=dev),
                 torch.empty(ecap + 1, dtype=index_dtype, device=dev) if coo else None,
                 torch.empty(ecap + 1, dtype=torch.int64, device=dev) if edge_ids else None)
            torch.cuda.current_stream(dev).synchronize()  # the tensors are the plan's stream's from here on
            return t

        if cap is None:
            _lib.check(call(0, 0, (None,) * 6), "plan_subgraphs")
            ncap, ecap = int(node_ptr[-1]), int(edge_ptr[-1])
        else:
            ncap, ecap = S * min(sz or self.L, self.L), cap
        t = alloc(ncap, ecap)
        rc = call(ncap, ecap, t)
        if rc == 11 and cap is not None and (int(node_ptr[-1]) > ncap or int(edge_ptr[-1]) > ecap):
            ncap, ecap = int(node_ptr[-1]), int(edge_ptr[-1])  # (the refused call completed both host arrays)
            t = alloc(ncap, ecap)
            rc = call(ncap, ecap, t)
        _lib.check(rc, "plan_subgraphs")
        N, E = int(node_ptr[-1]), int(edge_ptr[-1])
        if stats is not None:
            stats.update(device_ms=float(st.device_ms), edges_walked=int(st.edges_walked), edges=int(st.edges),
                         nodes=int(st.nodes), capped_members=int(st.capped_members), algo_bytes=int(st.algo_bytes),
                         wave_sources=int(st.wave_sources), wg_sources=int(st.wg_sources),
                         slice_sources=int(st.slice_sources), chunks=int(st.chunks))
        nodes_t, sc_t, rowptr_t, col_t, row_t, eid_t = t
        return SubgraphBatch(nodes_t[:N], None if sc_t is None else sc_t[:N], rowptr_t[:N + 1], col_t[:E],
                             None if row_t is None else row_t[:E], None if eid_t is None else eid_t[:E], node_ptr, edge_ptr)

    # ---- node-pair scores (include/ppr_hip.h ppr_grank_plan_pairs) ----
    def _pairs(self, gptr, src, cands, what, iterations_run, stats) -> PairResult:
        names = pair_outputs(what)
        Q, P = len(src), len(cands)
        it = self.iterations_run if iterations_run is None else iterations_run
        out = {"fwd": np.zeros(P, dtype=np.float64) if "fwd" in names else None,
               "bwd": np.zeros(P, dtype=np.float64) if "bwd" in names else None,
               "rank": np.full(P, -1, dtype=np.int32) if "rank" in names else None,
               "common": np.zeros(P, dtype=np.int32) if "common" in names else None,
               "dot": np.zeros(P, dtype=np.float64) if "dot" in names else None}
        hit = np.zeros(P, dtype=np.uint8)
        slen = np.zeros(Q, dtype=np.int32)
        clen = np.zeros(P, dtype=np.int32)
        st = _lib.PprPairsStats()
        # a pointer for empty arrays too: the C call refuses null pointers, and reads nothing through them
        dummy = np.zeros(1, dtype=np.int64)
        p = lambda a: None if a is None else (_lib.ptr(a) if a.size else _lib.ptr(dummy))
        _lib.check(_lib.lib().ppr_grank_plan_pairs(self._p, it, Q, _lib.ptr(gptr), p(src), p(cands), 0, p(out["fwd"]),
                                                   p(out["bwd"]), p(hit), p(out["rank"]), p(out["common"]), p(out["dot"]),
                                                   p(slen), p(clen), ctypes.byref(st)), "plan_pairs")
        if stats is not None:
            stats.update(device_ms=float(st.device_ms), **{f: int(getattr(st, f)) for f in (
                "pairs", "groups", "lookup_pairs", "overlap_pairs", "entries_read", "algo_bytes", "wave_groups", "wg_groups",
                "split_groups", "chunks")})
        return PairResult(src, cands, gptr, hit, slen, clen, **out)

    def pairs(self, sources, candidates, what=PAIR_OUTPUTS, iterations_run: Optional[int] = None,
              stats: Optional[dict] = None) -> PairResult:
        """Scores of node pairs from the plan's resident baskets, on the device (include/ppr_hip.h
        ppr_grank_plan_pairs): source sources[q] against each of its candidates. `candidates`: a sequence of
        candidate sequences, one per source, or a (gptr, cands) CSR; `what`: some of "fwd" (B[u][v]), "bwd"
        (B[v][u]), "rank" (the position of v in B[u] by score, for Hits@K and MRR), "common" (keys the rows
        share) and "dot" (their exact dot product); the hit bits and both row lengths come with any of
        them. Without "common" and "dot" only one 1/64 segment of a row is read per lookup. stats: a dict
        that receives the call's ppr_pairs_stats."""
        gptr, src, cands = normalize_groups(sources, candidates)
        return self._pairs(gptr, src, cands, what, iterations_run, stats)

    def pair_scores(self, u, v, what=PAIR_OUTPUTS, iterations_run: Optional[int] = None,
                    stats: Optional[dict] = None) -> PairResult:
        """pairs() for flat arrays: pair i is (u[i], v[i]). The pairs are grouped by source (a stable
        sort, normalize_pairs) and the results scattered back: every per-pair array of the result is in
        the caller's order, `sources` is u, `candidates` v, and every pair is a group of its own
        (gptr = 0, 1, 2, ...)."""
        gptr, src, cands, order, inverse = normalize_pairs(u, v)
        r = self._pairs(gptr, src, cands, what, iterations_run, stats)
        back = lambda a: None if a is None else np.ascontiguousarray(a[inverse])
        n = len(inverse)
        return PairResult(np.ascontiguousarray(r.pair_sources[inverse]), back(r.candidates), np.arange(n + 1, dtype=np.int64),
                          back(r.hit), np.ascontiguousarray(r.pair_src_len[inverse]), back(r.cand_len), back(r.fwd),
                          back(r.bwd), back(r.rank), back(r.common), back(r.dot))

    # ---- feature propagation (include/ppr_hip.h ppr_grank_plan_propagate / _propagate_t) ----
    @property
    def device(self) -> int:
        """HIP device ordinal the plan lives on"""
        d = ctypes.c_int32()
        _lib.check(_lib.lib().ppr_grank_plan_device(self._p, ctypes.byref(d)), "plan_device")
        return int(d.value)

    def _prop_sources(self, sources):
        """(S, int32 array or None) of a propagate call"""
        if sources is None:
            return self.csr.n, None
        try:
            import torch
            if isinstance(sources, torch.Tensor):
                sources = sources.detach().cpu().numpy()
        except ImportError:  # (a caller without torch passes arrays or lists)
            pass
        flat = np.asarray(sources, dtype=np.int64).reshape(-1)
        if len(flat) and (flat.min() < -2**31 or flat.max() >= 2**31):
            raise ValueError("source ids must fit in int32")
        return len(flat), np.ascontiguousarray(flat, dtype=np.int32)

    def _prop_tensor(self, t, rows: int, what: str, dtype=None, cols=None):
        """every refusal of a feature tensor, before any C call: a wrong shape would be an
        out-of-bounds access on the device"""
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor on the plan's device")
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{what} is on {t.device}, the plan on device {self.device}")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{what} must be float32 or bfloat16, not {t.dtype}")
        if dtype is not None and t.dtype != dtype:
            raise TypeError(f"{what} is {t.dtype}, the input {dtype}")
        if t.dim() != 2:
            raise ValueError(f"{what} must be 2-D, not {t.dim()}-D")
        if t.shape[0] != rows:
            raise ValueError(f"{what} has {t.shape[0]} rows, expected {rows}")
        if cols is not None and t.shape[1] != cols:
            raise ValueError(f"{what} has {t.shape[1]} columns, expected {cols}")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{what}: rows must be contiguous (stride {t.stride(1)})")
        if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise ValueError(f"{what}: row stride {t.stride(0)} below its {t.shape[1]} columns")
        return t

    def _propagate(self, fn_name, X, in_rows, out_rows, S, src, normalize, iterations_run, out, stats):
        import torch
        X = self._prop_tensor(X, in_rows, "the input")
        F = int(X.shape[1])
        if out is None:
            out = torch.empty((out_rows, F), dtype=X.dtype, device=X.device)
        else:
            self._prop_tensor(out, out_rows, "out", X.dtype, F)
        X, out_raw = X.detach(), out.detach()  # (views of the same memory: nothing here is recorded)
        it = self.iterations_run if iterations_run is None else iterations_run
        dt = _lib.PPR_PROP_BF16 if X.dtype == torch.bfloat16 else _lib.PPR_PROP_F32
        st = _lib.PprPropStats()
        ldx = int(X.stride(0)) if X.shape[0] > 1 else max(F, 1)
        ldo = int(out_raw.stride(0)) if out_raw.shape[0] > 1 else max(F, 1)
        # a pointer for an empty tensor too: the C call refuses null pointers, and reads nothing through it
        xp = X.data_ptr() or out_raw.data_ptr() or 1
        op = out_raw.data_ptr() or xp
        torch.cuda.current_stream(X.device).synchronize()  # H / G are complete before the plan's stream reads them
        fn = getattr(_lib.lib(), fn_name)
        _lib.check(fn(self._p, it, S, _lib.ptr(src), F, dt, _lib.PPR_PROP_ROW_NORMALIZE if normalize else 0,
                      xp, ldx, op, ldo, ctypes.byref(st)), fn_name)
        if stats is not None:
            stats.update(device_ms=float(st.device_ms), postings=int(st.postings), algo_bytes=int(st.algo_bytes),
                         passes=int(st.passes), chunks=int(st.chunks))
        return out

    def propagate(self, H, sources=None, normalize: bool = False, iterations_run: Optional[int] = None, out=None,
                  stats: Optional[dict] = None):
        """Z = B[sources] H on the device: row i of the result aggregates the feature rows of the
        keys of source i's basket, weighted by their scores (`normalize`: by score / row sum), in
        fp64, rounded once to H's dtype (float32 or bfloat16). H: torch tensor [n, F] on the plan's
        device; sources: dense ids (None: every node, in order); out: optional [S, F] tensor of the
        same dtype (a row stride above F is fine); stats: a dict that receives the call's
        ppr_prop_stats. Returns the [S, F] tensor. The C call runs on the plan's stream and returns
        when it is done."""
        S, src = self._prop_sources(sources)
        return self._propagate("ppr_grank_plan_propagate", H, self.csr.n, S, S, src, normalize, iterations_run, out,
                               stats)

    def propagate_t(self, G, sources=None, normalize: bool = False, iterations_run: Optional[int] = None, out=None,
                    stats: Optional[dict] = None):
        """Y = B[sources]^T G, the adjoint of propagate(): G is [S, F], the result [n, F] (every row
        written; keys no source of the batch holds get zeros). Bitwise reproducible: per key the
        postings are summed in ascending position, in chunks of 512, without float atomics."""
        S, src = self._prop_sources(sources)
        return self._propagate("ppr_grank_plan_propagate_t", G, S, self.csr.n, S, src, normalize, iterations_run, out,
                               stats)


def propagate(plan: GrankPlan, H, sources=None, normalize: bool = False):
    """Differentiable plan.propagate(H, sources, normalize): a torch.autograd.Function whose
    backward is plan.propagate_t(grad, sources, normalize) with the iteration count captured at the
    forward. No gradient flows into the table."""
    import torch

    it = plan.iterations_run
    S, src = plan._prop_sources(sources)

    class _Propagate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, h):
            return plan.propagate(h, src, normalize, it)

        @staticmethod
        def backward(ctx, grad):
            if not grad.is_contiguous():
                grad = grad.contiguous()  # (an expanded cotangent, as .sum() produces)
            return plan.propagate_t(grad, src, normalize, it)

    return _Propagate.apply(H)
