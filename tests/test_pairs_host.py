"""Host: the surface of the node-pair scores (ppr_grank_plan_pairs) without a GPU: the header's
declarations and its definition of algo_bytes, the ctypes mirror, the exported symbol, the provenance
list, the refusal of a null plan, the grouping of flat pairs and the helpers of PairResult."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

grank = sys.modules["approximated_personalized_pagerank_amd.grank"]  # (the package's `grank` is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppr_hip.h")).read()


def stats_fields():
    body = re.search(r"typedef struct ppr_pairs_stats \{(.*?)\} ppr_pairs_stats;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, rest = decl.split(None, 1)
            out += [(ty, nm.strip()) for nm in rest.split(",")]
    return out


def test_header_declares_the_surface():
    assert re.search(r"\bint ppr_grank_plan_pairs\(ppr_plan\* p, int32_t iterations_run, int64_t Q, const int64_t\* gptr,\s+"
                     r"const int32_t\* sources, const int32_t\* cands, uint32_t flags,\s+double\* out_fwd, double\* out_bwd, "
                     r"uint8_t\* out_hit, int32_t\* out_rank,\s+int32_t\* out_common, double\* out_dot, int32_t\* out_slen, "
                     r"int32_t\* out_clen,\s+ppr_pairs_stats\* st\);", HEADER)
    assert [n for _, n in stats_fields()] == ["device_ms", "pairs", "groups", "lookup_pairs", "overlap_pairs", "entries_read",
                                              "algo_bytes", "wave_groups", "wg_groups", "split_groups", "chunks", "reserved"]
    assert [t for t, _ in stats_fields()] == ["double"] + ["int64_t"] * 9 + ["int32_t"] * 2
    # the definition of algo_bytes is stated, and so are the bound of the sum and the refusal of MC plans
    flat = " ".join(HEADER.split()).replace(" * ", " ")
    for text in ("per group task 12 len(u) + 128 for the row and its range index", "per pair 4 len(v) for the ids",
                 "8 common for the scores of the hits", "per pair 8 for the two range-index reads", "4 per id of the two probed segments",
                 "8 per hit score", "14 len(u) + 128 once per group", "+ 4 for the candidate id", "X < 2^95",
                 "MC plans are refused"):
        assert text in flat, text


def test_ctypes_mirror_matches_the_header():
    size = {"double": 8, "int64_t": 8, "int32_t": 4}
    fields = stats_fields()
    assert ctypes.sizeof(_lib.PprPairsStats) == sum(size[t] for t, _ in fields) == 88
    assert [f[0] for f in _lib.PprPairsStats._fields_] == [name for _, name in fields]
    ctype = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [f[1] for f in _lib.PprPairsStats._fields_] == [ctype[t] for t, _ in fields]


def test_library_exports_and_provenance():
    assert "pairs.hip" in _lib.CSRC_SOURCES
    assert "pairs.h" in _lib.CSRC_HEADERS and "pairs_plan.h" in _lib.CSRC_HEADERS
    L = _lib.lib()
    assert L.ppr_grank_plan_pairs is not None and len(L.ppr_grank_plan_pairs.argtypes) == 16
    assert "PairResult" in ppr.__all__ and "normalize_pairs" in ppr.__all__
    assert callable(ppr.GrankPlan.pairs) and callable(ppr.GrankPlan.pair_scores)


def test_null_plan_is_refused():
    L = _lib.lib()
    st = _lib.PprPairsStats()
    st.pairs = 5
    gptr = np.array([0, 1], dtype=np.int64)
    ids = np.array([0], dtype=np.int32)
    fwd = np.full(1, -7.0)
    slen = np.full(1, -7, dtype=np.int32)
    args = (0, 1, _lib.ptr(gptr), _lib.ptr(ids), _lib.ptr(ids), 0, _lib.ptr(fwd), None, None, None, None, None, _lib.ptr(slen), None)
    assert L.ppr_grank_plan_pairs(None, *args, ctypes.byref(st)) == 1
    assert st.pairs == 0  # (the stats are cleared even by a refused call)
    assert fwd[0] == -7.0 and slen[0] == -7
    assert L.ppr_grank_plan_pairs(None, *args, None) == 1


def test_normalize_pairs():
    u = np.array([3, 1, 3, 2, 1, 3], dtype=np.int64)
    v = np.array([9, 8, 7, 6, 5, 9], dtype=np.int64)
    gptr, src, cands, order, inverse = ppr.normalize_pairs(u, v)
    assert gptr.dtype == np.int64 and src.dtype == np.int32 and cands.dtype == np.int32
    assert gptr.tolist() == [0, 2, 3, 6] and src.tolist() == [1, 2, 3]
    assert cands.tolist() == [8, 5, 6, 9, 7, 9]  # equal sources keep the caller's order of candidates
    assert order.tolist() == [1, 4, 3, 0, 2, 5]
    # the inverse permutation scatters back
    assert np.array_equal(cands[inverse], v) and np.array_equal(np.repeat(src, np.diff(gptr))[inverse], u)
    assert np.array_equal(order[inverse], np.arange(6)) and np.array_equal(inverse[order], np.arange(6))
    # lists, and a source of one pair
    g2, s2, c2, o2, i2 = ppr.normalize_pairs([5], [5])
    assert (g2.tolist(), s2.tolist(), c2.tolist(), o2.tolist(), i2.tolist()) == ([0, 1], [5], [5], [0], [0])
    # empty input
    g0, s0, c0, o0, i0 = ppr.normalize_pairs([], [])
    assert g0.tolist() == [0] and len(s0) == len(c0) == len(o0) == len(i0) == 0 and g0.dtype == np.int64
    rng = np.random.default_rng(1)
    u, v = rng.integers(0, 50, size=1000), rng.integers(0, 1000, size=1000)
    gptr, src, cands, order, inverse = ppr.normalize_pairs(u, v)
    assert np.all(np.diff(src) > 0) and gptr[0] == 0 and gptr[-1] == 1000 and np.all(np.diff(gptr) > 0)
    for q in (0, 7, len(src) - 1):
        assert cands[gptr[q]:gptr[q + 1]].tolist() == v[u == src[q]].tolist()
    assert np.array_equal(cands[inverse], v)
    for bad in (([1, 2], [1]), ([[1, 2]], [[1, 2]]), ([1], [[1]]), ([2**31], [0]), ([0], [-2**31 - 1])):
        with pytest.raises(ValueError):
            ppr.normalize_pairs(*bad)


def test_normalize_groups_and_outputs():
    gptr, src, cands = grank.normalize_groups([4, 2, 4], [[1, 2], [], [3]])
    assert (gptr.tolist(), src.tolist(), cands.tolist()) == ([0, 2, 2, 3], [4, 2, 4], [1, 2, 3])
    g2, s2, c2 = grank.normalize_groups(np.array([4, 2]), (np.array([0, 1, 3]), np.array([7, 8, 9])))
    assert (g2.tolist(), s2.tolist(), c2.tolist()) == ([0, 1, 3], [4, 2], [7, 8, 9]) and c2.dtype == np.int32
    for bad in (([1, 2], [[1]]), ([1], (np.array([0, 2]), np.array([7]))), ([1], (np.array([1, 1]), np.array([7])))):
        with pytest.raises(ValueError):
            grank.normalize_groups(*bad)
    assert grank.pair_outputs(("dot", "fwd")) == ("fwd", "dot") and grank.pair_outputs("rank") == ("rank",)
    for bad in ((), ("fwd", "jaccard"), "hit"):
        with pytest.raises(ValueError):
            grank.pair_outputs(bad)


def test_pair_result_helpers():
    # two groups: source 7 against (3, 7, 9), source 2 against (7)
    r = ppr.PairResult(sources=np.array([7, 2], dtype=np.int32), candidates=np.array([3, 7, 9, 7], dtype=np.int32),
                       gptr=np.array([0, 3, 4], dtype=np.int64), hit=np.array([3, 3, 0, 1], dtype=np.uint8),
                       src_len=np.array([4, 0], dtype=np.int32), cand_len=np.array([2, 4, 0, 4], dtype=np.int32),
                       fwd=np.array([0.25, 0.5, 0.0, 0.125]), common=np.array([2, 4, 0, 0], dtype=np.int32),
                       dot=np.array([0.125, 0.5, 0.0, 0.0]))
    assert r.pair_sources.tolist() == [7, 7, 7, 2] and r.pair_src_len.tolist() == [4, 4, 4, 0]
    assert r.jaccard().tolist() == [2 / 4, 1.0, 0.0, 0.0]  # (4 + 0 - 0 = 4 -> 0 / 4; 0 + 4 - 0 -> 0)
    # cosine: per-group or per-pair norms of u; a zero norm gives 0
    cs = r.cosine([0.5, 0.0], [0.125, 0.5, 0.0, 0.5])
    assert cs.tolist() == [0.125 / np.sqrt(0.5 * 0.125), 1.0, 0.0, 0.0]
    assert np.array_equal(r.cosine([0.5, 0.5, 0.5, 0.0], [0.125, 0.5, 0.0, 0.5]), cs)
    with pytest.raises(ValueError):
        r.cosine([0.5], [0.125, 0.5, 0.0, 0.5])
    # a denominator of 0: both rows empty
    e = ppr.PairResult(np.array([1], np.int32), np.array([1], np.int32), np.array([0, 1]), np.zeros(1, np.uint8),
                       np.zeros(1, np.int32), np.zeros(1, np.int32), common=np.zeros(1, np.int32))
    assert e.jaccard().tolist() == [0.0]
    with pytest.raises(ValueError):
        e.cosine([1.0], [1.0])
    with pytest.raises(ValueError):
        ppr.PairResult(r.sources, r.candidates, r.gptr, r.hit, r.src_len, r.cand_len, fwd=r.fwd).jaccard()
    g = ppr.Csr.from_dict({k: [] for k in "abcdefghij"})
    d = r.to_dicts(g)
    assert len(d) == 2 and set(d[0]) == {g.key(3), g.key(7), g.key(9)} and set(d[1]) == {g.key(7)}
    assert d[0][g.key(3)] == {"fwd": 0.25, "common": 2, "dot": 0.125, "hit": 3} and d[1][g.key(7)]["hit"] == 1
