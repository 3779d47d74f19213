"""Reverse queries, the parts that need no GPU: the ABI symbol, the flag and the stats struct in the
header, the refusal of a null plan, the provenance digest and the Python export."""
import ctypes
import os
import re

import numpy as np

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ppr_hip.h")


def test_header_declares_and_library_exports_rquery():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+ppr_grank_plan_rquery\s*\(", text)
    assert "PPR_RQUERY_EXCLUDE_TARGETS = 1" in text and "ppr_rquery_stats" in text
    assert _lib.PPR_RQUERY_EXCLUDE_TARGETS == 1
    assert hasattr(_lib.lib(), "ppr_grank_plan_rquery")


def test_rquery_source_is_part_of_the_digest():
    assert "rquery.hip" in _lib.CSRC_SOURCES
    assert "rquery.h" in _lib.CSRC_HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "rquery.hip"))


def test_null_plan_is_an_argument_error():
    qptr = np.zeros(1, dtype=np.int64)
    assert _lib.lib().ppr_grank_plan_rquery(None, 0, 0, _lib.ptr(qptr), None, None, 1, 0, None, None, None, None) == 1
    st = _lib.PprRQueryStats(device_ms=1.0, hits=5)
    assert _lib.lib().ppr_grank_plan_rquery(None, 0, 0, _lib.ptr(qptr), None, None, 1, 0, None, None, None,
                                            ctypes.byref(st)) == 1
    assert st.hits == 0 and st.device_ms == 0.0  # the stats are cleared even on a refusal


def test_stats_struct_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct ppr_rquery_stats \{(.*?)\} ppr_rquery_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"double": 8, "int64_t": 8, "int32_t": 4}
    names, total = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for nm in rest.split(","):
            names.append(nm.strip())
            total += size[ty]
    assert names == [f[0] for f in _lib.PprRQueryStats._fields_]
    assert ctypes.sizeof(_lib.PprRQueryStats) == total == 8 + 5 * 8 + 2 * 4


def test_rquery_result_is_exported():
    assert "RQueryResult" in ppr.__all__
    r = ppr.RQueryResult(np.array([[2, 0, -1]], dtype=np.int32), np.array([[0.5, 0.0, 0.0]]),
                         np.array([2], dtype=np.int32))
    g = ppr.Csr(np.array([0, 0, 0, 0]), np.zeros(0, dtype=np.int32), keys=["a", "b", "c"])
    assert r.to_dicts(g) == [{"c": 0.5, "a": 0.0}]
    assert (r.hits, r.scans, r.chunks, r.probe_queries, r.scan_queries) == (0, 0, 0, 0, 0)
    assert hasattr(ppr.GrankPlan, "rquery")
