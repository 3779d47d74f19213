"""Preference-set queries, the parts that need no GPU: the ABI symbol, its refusal of a null plan, the
Python export and the argument normalisation of GrankPlan.query (a plain function)."""
import os
import re

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib
from approximated_personalized_pagerank_amd.grank import normalize_queries

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ppr_hip.h")


def test_header_declares_and_library_exports_query():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+ppr_grank_plan_query\s*\(", text)
    assert "PPR_QUERY_EXCLUDE_SEEDS = 1" in text and "ppr_query_stats" in text
    assert hasattr(_lib.lib(), "ppr_grank_plan_query")
    assert "query.hip" in _lib.CSRC_SOURCES  # part of the provenance digest


def test_null_plan_is_an_argument_error():
    qptr = np.zeros(1, dtype=np.int64)
    assert _lib.lib().ppr_grank_plan_query(None, 0, 0, _lib.ptr(qptr), None, None, 1, 0, None, None, None, None) == 1


def test_query_result_is_exported():
    assert "QueryResult" in ppr.__all__
    r = ppr.QueryResult(np.array([[2, -1]], dtype=np.int32), np.array([[0.5, 0.0]]), np.array([1], dtype=np.int32))
    g = ppr.Csr(np.array([0, 0, 0, 0]), np.zeros(0, dtype=np.int32), keys=["a", "b", "c"])
    assert r.to_dicts(g) == [{"c": 0.5}]
    assert hasattr(ppr.GrankPlan, "query")


def test_stats_struct_matches_the_header():
    # double + 5 int64 + 2 int32
    import ctypes
    assert ctypes.sizeof(_lib.PprQueryStats) == 8 + 5 * 8 + 2 * 4


def test_lists_become_csr():
    qptr, seeds, w = normalize_queries([[3, 1], [], [7]])
    assert qptr.dtype == np.int64 and seeds.dtype == np.int32 and w is None
    assert qptr.tolist() == [0, 2, 2, 3] and seeds.tolist() == [3, 1, 7]
    qptr, seeds, w = normalize_queries([[3, 1], [], [7]], [[1, 2.5], [], [0]])
    assert w.dtype == np.float64 and w.tolist() == [1.0, 2.5, 0.0]
    # CSR arrays pass through; flat weights
    q2, s2, w2 = normalize_queries((np.array([0, 2, 2, 3]), np.array([3, 1, 7])), np.array([1, 2.5, 0]))
    assert q2.tolist() == qptr.tolist() and s2.tolist() == seeds.tolist() and w2.tolist() == w.tolist()
    assert q2.dtype == np.int64 and s2.dtype == np.int32
    qptr, seeds, w = normalize_queries([])
    assert qptr.tolist() == [0] and len(seeds) == 0


@pytest.mark.parametrize("queries,weights", [
    ([[1, 2], [3]], [[1.0, 2.0]]),                    # a row of weights missing
    ([[1, 2], [3]], [[1.0], [2.0]]),                  # a row too short
    ([[1, 2], [3]], [[1.0, 2.0], [3.0, 4.0]]),        # a row too long
    ([[1, 2], [3]], np.array([1.0, 2.0])),            # flat, too few
    ((np.array([0, 2, 3]), np.array([1, 2, 3])), np.ones(4)),
    ((np.array([0, 2, 4]), np.array([1, 2, 3])), None),   # qptr does not end at len(seeds)
    ((np.array([1, 2, 3]), np.array([1, 2, 3])), None),   # qptr does not start at 0
    ((np.array([0, 3, 2, 3]), np.array([1, 2, 3])), None),  # qptr decreases
])
def test_shape_mismatches_raise(queries, weights):
    with pytest.raises(ValueError):
        normalize_queries(queries, weights)
