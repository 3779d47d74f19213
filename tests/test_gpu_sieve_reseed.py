"""GPU: re-seeded retries of overflowed sieve sources (merge_sv.h).

A sieve source whose passing keys overflow its pass-2 table writes L seed keys (the top-L by value of
its prev table and the table's resident keys) and is retried once on the device with its prev table
built from them; only a second overflow reaches the host. Every case is bit-exact against the
oracle's exact sum on max_diff, lens, ids and scores, and the PPR_TIMING counters say which path ran:
sieve_reseed (seeded attempts), sieve_reseed_ok (those that completed), sieve_redo (host hand-backs).
Those counters sum the one-slice and the multi-slice sources, so the multi-slice cases also read the
per-iteration PPR_SV_LOG lines, which split the host hand-backs by class: hb_multi is the number of
multi-slice sources that reached the host.

The table budgets (PPR_SV_BUDGET, at least Lp so that seeds are written) make the first attempts of
these small graphs overflow; the counter conditions are conditions of the test. One-slice classes
run at 128 and 256. The multi-slice cases run at 128 and 192: with PPR_SV_SLICE=256 a slice holds at
most about 256 candidates, so a table of 256 keys can never overflow there (measured: 22-27 first
overflows at 128, 5-7 at 192, none at 256).
"""
import functools

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
import oracle

pytestmark = pytest.mark.gpu

CONFIGS = [(11, 16, 32, 8), (12, 32, 128, 6), (13, 64, 128, 5)]
L96 = [(12, 32, 96, 6)]  # Lp = 128 != L: seeds written and read at the padded stride

LARGE = {"PPR_SV_SMALL": "0", "PPR_SV_MID": "0", "PPR_TIER_MASK": "0x0"}  # every one-slice source 16 waves
SMALL = {"PPR_SV_SMALL": "1000000000", "PPR_SV_MID": "1000000000", "PPR_TIER_MASK": "0x0"}  # 4 waves, redo at 8
MID = {"PPR_SV_SMALL": "0", "PPR_SV_MID": "1000000000", "PPR_TIER_MASK": "0x0", "PPR_SV_REDO_LARGE": "1"}  # 8, redo at 16
MULTI = {"PPR_SV_SLICE": "256"}
MULTI_ALL = {"PPR_SV_SLICE": "256", "PPR_TIER_MASK": "0x0"}
KNOBS = ["PPR_SV_SMALL", "PPR_SV_MID", "PPR_TIER_MASK", "PPR_SV_REDO_LARGE", "PPR_SV_SLICE", "PPR_SV_BUDGET",
         "PPR_SV_RESEED", "PPR_SV_RESEED_BUDGET"]


@functools.lru_cache(maxsize=None)
def graph(scale):
    g = ppr.rmat(scale, seed=191 + scale)
    return g, g.partitions()


@functools.lru_cache(maxsize=None)
def reference(scale, K, L, it):
    g, part = graph(scale)
    o = oracle.grank(g.row_ptr, g.col, part, K, L, it, 0.85, -1.0)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def run(env, monkeypatch, capfd, configs=CONFIGS):
    """the configs under `env`, each bit-exact against the oracle; the summed sieve counters"""
    for k in KNOBS:  # (a test may call this twice: nothing of the first call's settings stays)
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PPR_SV_MIN", "0")
    monkeypatch.setenv("PPR_TIMING", "1")
    monkeypatch.setenv("PPR_SV_LOG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    for scale, K, L, it in configs:
        g, part = graph(scale)
        r = ppr.grank_csr(g, K, L, it, 0.85, -1.0, part=part, device=0)
        o = reference(scale, K, L, it)
        assert np.array_equal(r.max_diff, o["max_diff"])
        assert np.array_equal(r.lens, o["lens"])
        assert np.array_equal(r.ids, o["ids"])
        assert np.array_equal(r.scores, o["scores"])
    err = capfd.readouterr().err
    c = {"sieve_sources": 0, "sieve_redo": 0, "sieve_redo_dev": 0, "sieve_reseed": 0, "sieve_reseed_ok": 0,
         "hb_multi": 0}
    for ln in err.splitlines():
        f = ln.split()
        if ln.startswith("ppr_timing sieve_sources"):
            for i in range(1, len(f) - 1, 2):
                c[f[i]] += int(f[i + 1])
        elif ln.startswith("ppr_sv_log"):  # "... hb_multi <sources> <candidates> ..."
            c["hb_multi"] += int(f[f.index("hb_multi") + 1])
    print("sieve counters", env, c)
    assert c["sieve_sources"] > 0
    return c


def with_budget(env, budget, **more):
    return dict(env, PPR_SV_BUDGET=str(budget), **more)


@pytest.mark.parametrize("budget", [128, 256])
def test_gpu_reseed_large_class(budget, monkeypatch, capfd):
    """every one-slice source in the 16-wave class: its overflows are retried with the same geometry
    (k_sv1_list on the class's stream), which they never were before"""
    c = run(with_budget(LARGE, budget), monkeypatch, capfd)
    assert c["sieve_reseed"] > 0 and c["sieve_reseed_ok"] > 0
    assert c["sieve_redo_dev"] == 0  # (counts the small / mid device redos only, as before)


@pytest.mark.parametrize("budget", [128, 256])
@pytest.mark.parametrize("cls", ["small", "mid"])
def test_gpu_reseed_small_and_mid_class(cls, budget, monkeypatch, capfd):
    """the 4-wave class with its device redo (k_sv1_redo, 8 waves) and the 8-wave class with
    PPR_SV_REDO_LARGE=1 (k_sv1_list, 16 waves): the redo builds its prev table from the seeds"""
    c = run(with_budget(SMALL if cls == "small" else MID, budget), monkeypatch, capfd)
    assert c["sieve_reseed"] > 0 and c["sieve_reseed_ok"] > 0
    assert c["sieve_redo_dev"] > 0


@pytest.mark.parametrize("budget", [128, 192])
@pytest.mark.parametrize("env", [MULTI, MULTI_ALL], ids=["slice256", "slice256_all"])
def test_gpu_reseed_multi_slice(env, budget, monkeypatch, capfd):
    """multi-slice sources: overflowed slices still flush their resident keys, k_svS seeds the
    source, and the k_svA -> k_svB -> k_svF chain runs again for the marked descriptors. With
    re-seeding off, multi-slice sources overflow and reach the host (hb_multi > 0); with it on none
    does, so every one of them completed in the retry chain."""
    off = run(with_budget(env, budget, PPR_SV_RESEED="0"), monkeypatch, capfd)
    assert off["hb_multi"] > 0 and off["sieve_reseed"] == 0
    c = run(with_budget(env, budget), monkeypatch, capfd)
    assert c["hb_multi"] == 0
    assert c["sieve_reseed_ok"] > 0


@pytest.mark.parametrize("env,budget", [(LARGE, 128), (LARGE, 256), (MULTI, 128), (MULTI, 192), (MULTI_ALL, 128),
                                        (MULTI_ALL, 192)],
                         ids=["large-128", "large-256", "slice256-128", "slice256-192", "slice256_all-128",
                              "slice256_all-192"])
def test_gpu_reseed_second_overflow(env, budget, monkeypatch, capfd):
    """PPR_SV_RESEED_BUDGET=0: every seeded attempt overflows again and reaches the host hand-back"""
    c = run(with_budget(env, budget, PPR_SV_RESEED_BUDGET="0"), monkeypatch, capfd)
    assert c["sieve_reseed"] > 0
    assert c["sieve_reseed_ok"] == 0
    assert c["sieve_redo"] > 0
    if "PPR_SV_SLICE" in env:  # (the multi-slice sources' second overflows among them)
        assert c["hb_multi"] > 0


@pytest.mark.parametrize("env", [LARGE, SMALL, MULTI_ALL], ids=["large", "small", "slice256_all"])
def test_gpu_reseed_switched_off(env, monkeypatch, capfd):
    """PPR_SV_RESEED=0: no seeds, no seeded attempt -- the overflows go where they went before"""
    c = run(with_budget(env, 128, PPR_SV_RESEED="0"), monkeypatch, capfd)
    assert c["sieve_reseed"] == 0 and c["sieve_reseed_ok"] == 0
    assert c["sieve_redo"] > 0


@pytest.mark.parametrize("env", [LARGE, SMALL, MULTI_ALL], ids=["large", "small", "slice256_all"])
def test_gpu_reseed_padded_row(env, monkeypatch, capfd):
    """L = 96 at RMAT-12 (Lp = 128): the seeds are L keys in a row slot of Lp"""
    c = run(with_budget(env, 128), monkeypatch, capfd, configs=L96)
    assert c["sieve_reseed"] > 0 and c["sieve_reseed_ok"] > 0


def test_gpu_reseed_below_lp_keeps_old_path(monkeypatch, capfd):
    """a table budget below Lp holds too few keys to improve on the prev table: no seeds are written"""
    c = run(with_budget(LARGE, 40), monkeypatch, capfd, configs=CONFIGS[1:])
    assert c["sieve_reseed"] == 0
    assert c["sieve_redo"] > 0
