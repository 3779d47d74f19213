"""The long-double restatement of exact PPR (tests/exact_ref.py) pinned to the reference program's
recorded pprSingleSource vectors, and the host-only ends of the quality harness. No GPU."""
import ctypes

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
import exact_ref
from helpers import load

FULL = ["g5_ring100_full", "g5_instar_full", "g5_instar_loop_full", "g5_instar_all_full", "g5_random5000_full",
        "g5_complete_full", "m2_random100_full"]


@pytest.mark.parametrize("name", FULL)
def test_exact_ref_vs_reference_full_rows(name):
    """every source of a 100-node graph, 100 iterations, no tolerance stop, whole vectors"""
    f = load(name)
    z = f["z"]
    n = len(f["rp"]) - 1
    ref = exact_ref.exact_ppr(f["rp"], f["col"], np.arange(n), 0.85, 100, -1.0)
    assert (ref.iters == 100).all() and ref.diffs.shape == (100, n)
    ids, sc, cnt = exact_ref.top_rows(ref.f64, n)
    assert np.array_equal(cnt, z["pprss_cnt"])
    exact_ref.check_rows(ids, sc, cnt, z["pprss_ids"], z["pprss_scores"], z["pprss_cnt"])


def test_exact_ref_vs_reference_sampled_with_tolerance_stop():
    """the harness's own call pprSingleSource(g, 100, .85, 1e-4, v): the first 32 recorded sources of
    RMAT-12, each stopped by its own diff"""
    f = load("g3_rmat12_k16_l32")
    z = f["z"]
    src = z["pprss_src"][:32]
    kk = z["pprss_ids"].shape[1]
    ref = exact_ref.exact_ppr(f["rp"], f["col"], src, 0.85, 100, 1e-4)
    assert ref.iters.max() < 100 and len(set(ref.iters.tolist())) > 1  # the stop rule is what runs here
    ids, sc, cnt = exact_ref.top_rows(ref.f64, kk)
    assert np.array_equal(cnt, z["pprss_cnt"][:32])
    rc = np.minimum(cnt, kk)
    exact_ref.check_rows(ids, sc, rc, z["pprss_ids"][:32], z["pprss_scores"][:32], rc)


def test_exact_ref_stop_rule_by_hand():
    """0 -> 1 -> 2 (dangling), d = 0.5, source 0: x1 = (.5, .5, 0), x2 = (.5, .25, .25),
    x3 = (.5, .25, .125) = x4; diffs 1, .5, .125, 0; a dangling source stops at 2 with (1 - d) e_s"""
    rp, col = np.array([0, 1, 2, 2]), np.array([1, 2])
    r = exact_ref.exact_ppr(rp, col, [0, 2], 0.5, 100, 1e-4)
    assert r.iters.tolist() == [4, 2]
    assert r.f64[:, 0].tolist() == [0.5, 0.25, 0.125] and r.f64[:, 1].tolist() == [0.0, 0.0, 0.5]
    assert r.diffs[:, 0].astype(float).tolist() == [1.0, 0.5, 0.125, 0.0]
    assert r.diffs[:2, 1].astype(float).tolist() == [0.5, 0.0] and np.isnan(r.diffs[2:, 1].astype(float)).all()
    assert exact_ref.exact_ppr(rp, col, [0], 0.5, 2, 1e-4).iters.tolist() == [2]       # the iteration cap
    # a repeated edge counts once per repetition: 0 -> [1, 1, 2]
    r = exact_ref.exact_ppr(np.array([0, 3, 3, 3]), np.array([1, 1, 2]), [0], 0.75, 1, -1.0)
    assert r.f64[:, 0].tolist() == [0.25, 0.5, 0.25]


def test_benchmark_algorithm_refuses_zero_test_nodes():
    g = ppr.Csr([0, 1, 2], [1, 0])
    with pytest.raises(ValueError):
        ppr.benchmark_algorithm({0: {1: 0.5}}, g, 0, False)
    with pytest.raises(ValueError):
        exact_ref.benchmark_ref({0: {1: 0.5}}, g, 0, False)


def test_benchmark_algorithm_strict_with_only_dangling_sources():
    """strict drops every source without successors; nothing is left to sample: -1 five times
    (include/benchmarkAlgorithm.h:144-151), before any exact run"""
    g = ppr.Csr.from_dict({"a": ["b", "c"], "b": [], "c": []})
    res = {"b": {"b": 0.15}, "c": {"c": 0.15, "a": 0.0}}
    q = ppr.benchmark_algorithm(res, g, 5, True, seed=0)
    assert q == {k: -1.0 for k in exact_ref.FIGURES}
    assert exact_ref.benchmark_ref(res, g, 5, True) == q


def test_benchmark_ref_by_hand():
    """0 -> 1 -> 2 (dangling), exact column of 0 = (.15, .1275, .108375) after the stop"""
    g = ppr.Csr([0, 1, 2, 2], [1, 2])
    q = exact_ref.benchmark_ref({0: {0: 0.9, 2: 0.5}, 2: {2: 1.0}}, g, 2, False)
    # source 0: keepTop(2) = {0, 1} against {0, 2} -> 1/3, the two looked-up scores agree in order -> 1
    assert q["jaccard average"] == pytest.approx((1 / 3 + 1) / 2, abs=1e-15) and q["jaccard min"] == pytest.approx(1 / 3)
    assert q["kendall average"] == 1.0 and q["kendall min"] == 1.0 and q["average map size"] == 1.5
    q = exact_ref.benchmark_ref({0: {0: 0.1, 2: 0.5}, 2: {2: 1.0}}, g, 2, True)
    assert q["kendall min"] == -1.0 and q["average map size"] == 2.0 and q["jaccard average"] == pytest.approx(1 / 3)


@pytest.mark.parametrize("shape", [(3,), (2, 4), (4, 4), (0, 4), (3, 2, 2)])
def test_gather_refuses_keys_of_another_shape(shape, monkeypatch):
    """keys must be [len(sources), Q]: the library copies len(sources) * Q entries in and out, so any
    other shape would run past the host arrays. Refused before the library is touched."""
    ex = object.__new__(ppr.ExactPPR)
    ex.sources = np.arange(3, dtype=np.int32)
    ex._h = ctypes.c_void_p()

    def no_library():
        raise AssertionError("gather reached the library")
    monkeypatch.setattr(ppr._lib, "lib", no_library)
    with pytest.raises(ValueError):
        ex.gather(np.zeros(shape, dtype=np.int32))
