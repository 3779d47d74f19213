"""Host: the surface of the sweep cuts (ppr_grank_plan_sweep / ppr_grank_plan_sweep_vectors) without
a GPU: the header's declarations, the ctypes mirror, the exported symbols, the provenance list and
the refusals that need no device."""
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
    body = re.search(r"typedef struct ppr_sweep_stats \{(.*?)\} ppr_sweep_stats;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, rest = decl.split(None, 1)
            out += [(ty, nm.strip()) for nm in rest.split(",")]
    return out


def test_header_declares_the_surface():
    for name in ("ppr_grank_plan_sweep", "ppr_grank_plan_sweep_vectors"):
        assert re.search(r"\bint " + name + r"\(ppr_plan\* p,", HEADER), name
    tail = (r"uint32_t min_size,\s+uint32_t max_size, int64_t max_vol, uint32_t flags,\s+int32_t\* out_order,\s+"
            r"int32_t\* out_swept, int32_t\* out_size, int64_t\* out_cut,\s+int64_t\* out_vol,\s+double\* out_phi, "
            r"int64_t\* prof_cut, int64_t\* prof_vol,\s+ppr_sweep_stats\* st\);")
    assert re.search(r"ppr_grank_plan_sweep\(ppr_plan\* p, int32_t iterations_run, int64_t S, const int32_t\* sources,\s+" + tail,
                     HEADER)
    assert re.search(r"ppr_grank_plan_sweep_vectors\(ppr_plan\* p, int64_t R, int32_t width_in, const int32_t\* ids,\s+"
                     r"const double\* scores, const int32_t\* lens, " + tail, HEADER)
    assert stats_fields() == [("double", "device_ms"), ("int64_t", "edges"), ("int64_t", "algo_bytes"),
                              ("int64_t", "wave_sources"), ("int64_t", "wg_sources"), ("int64_t", "slice_sources"),
                              ("int32_t", "chunks"), ("int32_t", "reserved")]
    # the definition of algo_bytes is stated
    assert "per row entry 28" in HEADER and "per walked edge 4" in HEADER and "per source 4 * width + 36" in HEADER


def test_ctypes_mirror_matches_the_header():
    size = {"double": 8, "int64_t": 8, "int32_t": 4}
    fields = stats_fields()
    assert ctypes.sizeof(_lib.PprSweepStats) == sum(size[t] for t, _ in fields) == 56
    assert [f[0] for f in _lib.PprSweepStats._fields_] == [name for _, name in fields]
    ctype = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [f[1] for f in _lib.PprSweepStats._fields_] == [ctype[t] for t, _ in fields]


def test_library_exports_and_provenance():
    assert "sweep.hip" in _lib.CSRC_SOURCES
    assert "sweep.h" in _lib.CSRC_HEADERS and "sweep_plan.h" in _lib.CSRC_HEADERS
    # the digest covers the new files: it changes with their contents
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        inc = os.path.join(tmp, "pkg", "csrc")
        shutil.copytree(_lib.CSRC, inc)
        os.makedirs(os.path.join(tmp, "include"))
        shutil.copy(os.path.join(ROOT, "include", "ppr_hip.h"), os.path.join(tmp, "include"))
        assert _lib.source_digest(inc) == _lib.source_digest()
        for f in ("sweep.hip", "sweep.h", "sweep_plan.h"):
            before = _lib.source_digest(inc)
            with open(os.path.join(inc, f), "a") as fh:
                fh.write("// x\n")
            assert _lib.source_digest(inc) != before, f
    L = _lib.lib()
    for name in ("ppr_grank_plan_sweep", "ppr_grank_plan_sweep_vectors"):
        assert getattr(L, name) is not None
    assert len(L.ppr_grank_plan_sweep.argtypes) == 17 and len(L.ppr_grank_plan_sweep_vectors.argtypes) == 19


def test_null_plan_is_refused():
    L = _lib.lib()
    st = _lib.PprSweepStats()
    st.edges = 5
    o32, o64, of = np.full(4, -7, np.int32), np.full(4, -7, np.int64), np.full(4, -7.0)
    assert L.ppr_grank_plan_sweep(None, 0, 1, _lib.ptr(o32), 1, 0, 0, 0, _lib.ptr(o32), _lib.ptr(o32), _lib.ptr(o32),
                                  _lib.ptr(o64), _lib.ptr(o64), _lib.ptr(of), None, None, ctypes.byref(st)) == 1
    assert st.edges == 0  # (the stats are cleared even by a refused call)
    assert L.ppr_grank_plan_sweep_vectors(None, 1, 4, _lib.ptr(o32), _lib.ptr(of), _lib.ptr(o32), 1, 0, 0, 0, _lib.ptr(o32),
                                          _lib.ptr(o32), _lib.ptr(o32), _lib.ptr(o64), _lib.ptr(o64), _lib.ptr(of), None,
                                          None, None) == 1
    assert np.all(o32 == -7) and np.all(o64 == -7) and np.all(of == -7.0)


def test_names_are_exported():
    assert "SweepResult" in ppr.__all__
    assert callable(ppr.GrankPlan.sweep) and callable(ppr.GrankPlan.sweep_vectors)
    r = ppr.SweepResult(np.array([[2, 0, 1, -1], [1, -1, -1, -1]], dtype=np.int32), np.array([3, 1], dtype=np.int32),
                        np.array([2, 0], dtype=np.int32), np.array([1, 0]), np.array([4, 0]), np.array([0.25, np.inf]))
    assert [s.tolist() for s in r.sets()] == [[2, 0], []] and r.sets()[0].dtype == np.int32
    g = ppr.Csr(np.array([0, 0, 0, 0]), np.zeros(0, dtype=np.int32), keys=["a", "b", "c"])
    assert r.to_dicts(g) == [{"c": 0, "a": 1}, {}]
    assert r.profile_cut is None and r.profile_vol is None


def test_python_refusals_need_no_device():
    ids = np.array([[3, 1, -1], [2, -1, -1]])
    sc = np.array([[0.5, 0.25, 0.0], [1.0, 0.0, 0.0]])
    a, b, c = grank.normalize_vectors(ids, sc)
    assert a.dtype == np.int32 and b.dtype == np.float64 and c.dtype == np.int32 and c.tolist() == [2, 1]
    assert grank.normalize_vectors(ids, sc, [3, 0])[2].tolist() == [3, 0]
    q = ppr.QueryResult(ids.astype(np.int32), sc, np.array([2, 1], dtype=np.int32))
    assert grank.normalize_vectors(q)[2].tolist() == [2, 1]
    full = grank.normalize_vectors(np.array([[1, 2]]), np.array([[0.5, 0.5]]))
    assert full[2].tolist() == [2]
    for bad in (lambda: grank.normalize_vectors(ids),                       # no scores
                lambda: grank.normalize_vectors(ids, sc[:, :2]),            # shapes differ
                lambda: grank.normalize_vectors(ids[0], sc[0]),             # not 2-D
                lambda: grank.normalize_vectors(ids, sc, [1]),              # lens of another length
                lambda: grank.normalize_vectors(q, lens=[1, 1]),            # lens twice
                lambda: grank.normalize_vectors(ids + 2**31, sc)):          # ids beyond int32
        with pytest.raises(ValueError):
            bad()
    assert grank.sweep_arguments(1, None, None) == (1, 0, 0)
    assert grank.sweep_arguments(3, 7, 64) == (3, 7, 64)
    for bad in ((-1, None, None), (1, -2, None), (1, 0, None), (2**32, None, None), (1, 2**32, None), (1, None, 2**63)):
        with pytest.raises(ppr.PprError) as e:
            grank.sweep_arguments(*bad)
        assert e.value.code == 1
