"""Host: the surface of the feature propagation (ppr_grank_plan_propagate / ppr_grank_plan_propagate_t)
without a GPU: the header's declarations, the ctypes mirror, the exported symbols, the provenance
list and the refusals that need no device."""
import ctypes
import os
import re

import approximated_personalized_pagerank_amd as ppr
from approximated_personalized_pagerank_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppr_hip.h")).read()


def test_header_declares_the_surface():
    for name in ("ppr_grank_plan_propagate", "ppr_grank_plan_propagate_t", "ppr_grank_plan_device"):
        assert re.search(r"\bint " + name + r"\(ppr_plan\* p,", HEADER), name
    assert re.search(r"enum \{ PPR_PROP_F32 = 0, PPR_PROP_BF16 = 1 \};", HEADER)
    assert re.search(r"enum \{ PPR_PROP_ROW_NORMALIZE = 1 \};", HEADER)
    assert re.search(r"#define PPR_PROP_CHUNK 512\b", HEADER)
    m = re.search(r"typedef struct ppr_prop_stats \{(.*?)\} ppr_prop_stats;", HEADER, re.S)
    assert m
    fields = re.findall(r"\b(double|int64_t|int32_t) (\w+);", m.group(1))
    assert fields == [("double", "device_ms"), ("int64_t", "postings"), ("int64_t", "algo_bytes"), ("int64_t", "passes"),
                      ("int32_t", "chunks"), ("int32_t", "reserved")]
    # the definition of algo_bytes is stated
    assert "per posting 12" in HEADER and "per position 8" in HEADER


def test_ctypes_mirror_matches_the_header():
    size = {"double": 8, "int64_t": 8, "int32_t": 4}
    m = re.search(r"typedef struct ppr_prop_stats \{(.*?)\} ppr_prop_stats;", HEADER, re.S)
    fields = re.findall(r"\b(double|int64_t|int32_t) (\w+);", m.group(1))
    assert ctypes.sizeof(_lib.PprPropStats) == sum(size[t] for t, _ in fields) == 40
    assert [f[0] for f in _lib.PprPropStats._fields_] == [name for _, name in fields]
    assert (_lib.PPR_PROP_F32, _lib.PPR_PROP_BF16, _lib.PPR_PROP_ROW_NORMALIZE, _lib.PPR_PROP_CHUNK) == (0, 1, 1, 512)


def test_library_exports_and_provenance():
    assert "propagate.hip" in _lib.CSRC_SOURCES
    assert "propagate.h" in _lib.CSRC_HEADERS and "prop_plan.h" in _lib.CSRC_HEADERS
    L = _lib.lib()
    for name in ("ppr_grank_plan_propagate", "ppr_grank_plan_propagate_t", "ppr_grank_plan_device"):
        assert getattr(L, name) is not None


def test_null_plan_is_refused():
    L = _lib.lib()
    st = _lib.PprPropStats()
    assert L.ppr_grank_plan_propagate(None, 0, 0, None, 8, 0, 0, None, 8, None, 8, ctypes.byref(st)) == 1
    assert L.ppr_grank_plan_propagate_t(None, 0, 0, None, 8, 0, 0, None, 8, None, 8, None) == 1
    d = ctypes.c_int32(-7)
    assert L.ppr_grank_plan_device(None, ctypes.byref(d)) == 1


def test_names_are_exported():
    assert "propagate" in ppr.__all__ and callable(ppr.propagate)
    assert callable(ppr.GrankPlan.propagate) and callable(ppr.GrankPlan.propagate_t)
