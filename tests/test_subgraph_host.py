"""Host: the surface of the induced subgraph batches (ppr_grank_plan_subgraphs) without a GPU: the
header's declarations, the ctypes mirror, the exported symbol, the provenance list, the refusals
that need no device and the helpers of SubgraphBatch on CPU tensors."""
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
    body = re.search(r"typedef struct ppr_subg_stats \{(.*?)\} ppr_subg_stats;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, rest = decl.split(None, 1)
            out += [(ty, nm.strip()) for nm in rest.split(",")]
    return out


def test_header_declares_the_surface():
    assert re.search(r"enum \{ PPR_SUBG_ROOT_FIRST = 1, PPR_SUBG_IDX64 = 2 \};", HEADER)
    assert re.search(r"\bint ppr_grank_plan_subgraphs\(ppr_plan\* p, int32_t iterations_run, int64_t S, const int32_t\* sources,\s+"
                     r"uint32_t size, int64_t max_deg, uint32_t flags, int64_t node_cap,\s+int64_t edge_cap, "
                     r"int64_t\* node_ptr, int64_t\* edge_ptr, void\* nodes,\s+double\* scores, void\* rowptr, void\* col, "
                     r"void\* row, int64_t\* eid,\s+ppr_subg_stats\* st\);", HEADER)
    assert stats_fields() == [("double", "device_ms"), ("int64_t", "edges_walked"), ("int64_t", "edges"), ("int64_t", "nodes"),
                              ("int64_t", "capped_members"), ("int64_t", "algo_bytes"), ("int64_t", "wave_sources"),
                              ("int64_t", "wg_sources"), ("int64_t", "slice_sources"), ("int32_t", "chunks"),
                              ("int32_t", "reserved")]
    # the definition of algo_bytes is stated
    assert "row entry 12" in HEADER and "per walked edge 4 in the count pass" in HEADER and "per 64-edge group 8" in HEADER
    assert (_lib.PPR_SUBG_ROOT_FIRST, _lib.PPR_SUBG_IDX64) == (1, 2)


def test_ctypes_mirror_matches_the_header():
    size = {"double": 8, "int64_t": 8, "int32_t": 4}
    fields = stats_fields()
    assert ctypes.sizeof(_lib.PprSubgStats) == sum(size[t] for t, _ in fields) == 80
    assert [f[0] for f in _lib.PprSubgStats._fields_] == [name for _, name in fields]
    ctype = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [f[1] for f in _lib.PprSubgStats._fields_] == [ctype[t] for t, _ in fields]


def test_library_exports_and_provenance():
    assert "subgraph.hip" in _lib.CSRC_SOURCES
    assert "subgraph.h" in _lib.CSRC_HEADERS and "subgraph_plan.h" in _lib.CSRC_HEADERS
    # the digest covers the new files: it changes with their contents
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        inc = os.path.join(tmp, "pkg", "csrc")
        shutil.copytree(_lib.CSRC, inc)
        os.makedirs(os.path.join(tmp, "include"))
        shutil.copy(os.path.join(ROOT, "include", "ppr_hip.h"), os.path.join(tmp, "include"))
        assert _lib.source_digest(inc) == _lib.source_digest()
        for f in ("subgraph.hip", "subgraph.h", "subgraph_plan.h"):
            before = _lib.source_digest(inc)
            with open(os.path.join(inc, f), "a") as fh:
                fh.write("// x\n")
            assert _lib.source_digest(inc) != before, f
    L = _lib.lib()
    assert L.ppr_grank_plan_subgraphs is not None and len(L.ppr_grank_plan_subgraphs.argtypes) == 18


def test_null_plan_is_refused():
    L = _lib.lib()
    st = _lib.PprSubgStats()
    st.edges = 5
    src = np.array([0], dtype=np.int32)
    np_, ep = np.full(2, -7, np.int64), np.full(2, -7, np.int64)
    assert L.ppr_grank_plan_subgraphs(None, 0, 1, _lib.ptr(src), 0, 0, 0, 0, 0, _lib.ptr(np_), _lib.ptr(ep), None, None, None,
                                      None, None, None, ctypes.byref(st)) == 1
    assert st.edges == 0  # (the stats are cleared even by a refused call)
    assert np.all(np_ == -7) and np.all(ep == -7)
    assert L.ppr_grank_plan_subgraphs(None, 0, 1, _lib.ptr(src), 0, 0, 0, 0, 0, _lib.ptr(np_), _lib.ptr(ep), None, None, None,
                                      None, None, None, None) == 1


def test_python_refusals_need_no_device():
    assert grank.subgraph_arguments(None, None) == (0, 0, None)
    assert grank.subgraph_arguments(20, 100, 5000) == (20, 100, 5000)
    assert grank.subgraph_arguments(4096, None, 0) == (4096, 0, 0)
    for bad in ((-1, None, None), (0, None, None), (2**32, None, None), (None, -1, None), (None, 0, None), (None, 2**63, None),
                (None, None, -1), (None, None, 2**63)):
        with pytest.raises(ppr.PprError) as e:
            grank.subgraph_arguments(*bad)
        assert e.value.code == 1, bad
    with pytest.raises(ppr.PprError) as e:
        grank.subgraph_arguments(4097, None)
    assert e.value.code == 11
    # a wrong index type is refused before the plan or the device is touched
    import torch
    plan = object.__new__(ppr.GrankPlan)  # (no plan behind it: the check comes first)
    plan._p = ctypes.c_void_p()
    for dt in (torch.int16, torch.float32, torch.uint8, np.int64, "int64"):
        with pytest.raises(TypeError):
            ppr.GrankPlan.subgraphs(plan, [0], index_dtype=dt)


def test_batch_helpers_on_cpu_tensors():
    import torch
    assert "SubgraphBatch" in ppr.__all__ and callable(ppr.GrankPlan.subgraphs)
    # three positions: members {7, 3, 9}, {} and {3, 4}
    b = ppr.SubgraphBatch(nodes=torch.tensor([7, 3, 9, 3, 4]), scores=torch.tensor([0.5, 0.25, 0.125, 0.75, 0.25], dtype=torch.float64),
                          rowptr=torch.tensor([0, 2, 2, 3, 4, 5]), col=torch.tensor([1, 2, 0, 4, 3]),
                          row=torch.tensor([0, 0, 2, 3, 4]), eid=None, node_ptr=np.array([0, 3, 3, 5]),
                          edge_ptr=np.array([0, 3, 3, 5]))
    assert (b.num_graphs, b.num_nodes, b.num_edges) == (3, 5, 5)
    assert b.edge_index.shape == (2, 5) and b.edge_index.tolist() == [[0, 0, 2, 3, 4], [1, 2, 0, 4, 3]]
    assert b.roots.tolist() == [0, 3, 3] and b.roots.dtype == torch.int64
    assert b.batch.tolist() == [0, 0, 0, 2, 2] and b.batch.dtype == torch.int64
    no_coo = ppr.SubgraphBatch(b.nodes, None, b.rowptr, b.col, None, None, b.node_ptr, b.edge_ptr)
    with pytest.raises(ValueError):
        no_coo.edge_index
    empty = ppr.SubgraphBatch(torch.zeros(0, dtype=torch.int64), None, torch.zeros(1, dtype=torch.int64),
                              torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), None, np.zeros(1, np.int64),
                              np.zeros(1, np.int64))
    assert empty.num_graphs == 0 and empty.batch.shape == (0,) and empty.roots.shape == (0,) and empty.edge_index.shape == (2, 0)
