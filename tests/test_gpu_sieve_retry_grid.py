"""GPU: the sieve's retry grids from the partition's overflow history, and seedless attempts of
short-row sources (merge_sv.h, sv_plan.h).

The retry launch behind a class (k_sv1_list, or the second multi-slice chain) is sized on the host:
the whole class at a partition's first sieved update of a job, 2 * (last update's first overflows)
+ 64 later, and no launch at all after two updates without an overflow (PPR_SV_RETRY_GRID: auto |
legacy | full | N). A source whose current row is short runs a first attempt with theta = 0 where a
seeded retry stands behind its launch (PPR_SV_SEEDLESS). Neither may change a bit of the result:
every run here is bit-exact against the oracle's exact sum on max_diff, lens, ids and scores, and the
counters say which path ran -- the `ppr_timing sieve_sources` line as in test_gpu_sieve_reseed.py,
the new `ppr_timing sieve_retry` line (launched / skipped: retry launches or chains queued and
skipped; past_grid: first overflows that found no retry block; seedless / seedless_done: first
attempts without a full row, and such sources whose row the sieve wrote) and the per-update
PPR_SV_LOG lines, which carry the same five counters per call.

The counter conditions are conditions of the test. Measured on an MI355X, summed over the configs
of a case (the counts move by a few between runs: which slots a table's keys take decides the
borderline overflows):
  large class, budget 128 (19,908 sieved sources, 19 sieved updates): auto 4,580 seeded attempts, all
    complete, 18 launches queued and 1 skipped, past_grid 0, no host hand-back; PPR_SV_RETRY_GRID=1
    14 retried, past_grid 4,559 = sieve_redo; full 4,579 / 4,579; legacy 1,851 retried, 2,721 past
    the grid. (With the grid from the bare last count, 2,417 went past it in auto: a partition's
    second update takes many more sources than its first -- hence sv_scale_prev.)
  skip (RMAT-11, default budget): 8 updates, 4 launches queued, 4 skipped, no overflow.
  multi-slice, PPR_SV_SLICE=256: 23 / 5 seeded attempts at budgets 128 / 192, all complete, hb_multi
    0, the chain queued 14 times and skipped 5 (legacy: 19 and 0).
  seedless (four configs): 13,186 seedless attempts; rows written by the sieve 11,891 (small class,
    budget 128), 13,175 (large, 128), 13,181 / 13,185 (small / large, 256); 25,838 -> 39,024 sieved
    sources. At the default budget nothing overflows at RMAT-11 (1,343 attempts, 1,343 written).
    None with PPR_SV_RESEED=0 or budget 40.
  second run of one plan: 6 launches queued, none skipped, in both runs.
"""
import functools

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
import oracle

pytestmark = pytest.mark.gpu

CONFIGS = [(11, 16, 32, 8), (12, 32, 128, 6), (13, 64, 128, 5)]
L96 = [(12, 32, 96, 6)]  # Lp = 128 != L: seeds written and read at the padded stride
ALL = CONFIGS + L96

LARGE = {"PPR_SV_SMALL": "0", "PPR_SV_MID": "0", "PPR_TIER_MASK": "0x0"}  # every one-slice source 16 waves
SMALL = {"PPR_SV_SMALL": "1000000000", "PPR_SV_MID": "1000000000", "PPR_TIER_MASK": "0x0"}  # 4 waves, redo at 8
MULTI = {"PPR_SV_SLICE": "256"}
KNOBS = ["PPR_SV_SMALL", "PPR_SV_MID", "PPR_TIER_MASK", "PPR_SV_REDO_LARGE", "PPR_SV_SLICE", "PPR_SV_BUDGET",
         "PPR_SV_RESEED", "PPR_SV_RESEED_BUDGET", "PPR_SV_RETRY_GRID", "PPR_SV_SEEDLESS"]
RETRY_KEYS = ["launched", "skipped", "past_grid", "seedless", "seedless_done"]
LOG_KEYS = ["retry_launched", "retry_skipped", "past_grid", "seedless", "seedless_done"]


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


def counters(err):
    c = {"sieve_sources": 0, "sieve_redo": 0, "sieve_redo_dev": 0, "sieve_reseed": 0, "sieve_reseed_ok": 0,
         "hb_multi": 0, "updates": 0}
    c.update({k: 0 for k in RETRY_KEYS})
    c.update({"log_" + k: 0 for k in LOG_KEYS})
    for ln in err.splitlines():
        f = ln.split()
        if ln.startswith("ppr_timing sieve_sources") or ln.startswith("ppr_timing sieve_retry"):
            for i in range(2 if f[1] == "sieve_retry" else 1, len(f) - 1, 2):
                c[f[i]] += int(f[i + 1])
        elif ln.startswith("ppr_sv_log"):
            c["hb_multi"] += int(f[f.index("hb_multi") + 1])
            c["updates"] += int(f[f.index("sieved") + 1]) > 0
            for k in LOG_KEYS:
                c["log_" + k] += int(f[f.index(k) + 1])
    return c


def run(env, monkeypatch, capfd, configs=CONFIGS):
    """the configs under `env`, each bit-exact against the oracle; the summed sieve counters"""
    for k in KNOBS:
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
    c = counters(capfd.readouterr().err)
    print("sieve counters", env, c)
    assert c["sieve_sources"] > 0
    # the per-update log lines and the per-plan totals count the same things
    for k, lk in zip(RETRY_KEYS, LOG_KEYS):
        assert c[k] == c["log_" + lk]
    return c


def large128(**more):
    return dict(LARGE, PPR_SV_BUDGET="128", **more)


def test_gpu_retry_grid_auto_large_class(monkeypatch, capfd):
    """auto: the grid holds every first overflow (the whole class at a partition's first update,
    twice the last count + 64 later), so every host hand-back is a second overflow"""
    c = run(large128(), monkeypatch, capfd)
    assert c["sieve_reseed"] > 0 and c["launched"] > 0
    assert c["past_grid"] == 0
    assert c["sieve_redo"] == c["sieve_reseed"] - c["sieve_reseed_ok"]


def test_gpu_retry_grid_one_block(monkeypatch, capfd):
    """PPR_SV_RETRY_GRID=1: one retry block a launch -- the other first overflows go past the grid to
    the host (k_sv1_list's safety net), bit-exact all the same"""
    c = run(large128(PPR_SV_RETRY_GRID="1"), monkeypatch, capfd)
    assert c["past_grid"] > 0
    assert c["sieve_redo"] > 0
    assert c["sieve_reseed_ok"] <= c["launched"]


@pytest.mark.parametrize("mode", ["full", "legacy"])
def test_gpu_retry_grid_full_and_legacy(mode, monkeypatch, capfd):
    c = run(large128(PPR_SV_RETRY_GRID=mode), monkeypatch, capfd)
    assert c["sieve_reseed_ok"] > 0
    assert c["skipped"] == 0


def test_gpu_retry_grid_skips_without_overflows(monkeypatch, capfd):
    """RMAT-11 has 2,048 nodes: a source has at most 2,048 distinct keys, below the large class's
    budget of 2,457, so nothing can overflow. After a partition's second update without an overflow
    the retry launch is skipped: at most two launches per partition"""
    c = run(LARGE, monkeypatch, capfd, configs=CONFIGS[:1])
    assert c["sieve_reseed"] == 0
    assert c["skipped"] > 0
    assert c["launched"] <= 2 * 2
    assert c["past_grid"] == 0 and c["sieve_redo"] == 0


@pytest.mark.parametrize("budget", [128, 192])
@pytest.mark.parametrize("mode", ["auto", "legacy"])
def test_gpu_retry_grid_multi_slice(mode, budget, monkeypatch, capfd):
    """the second k_svA -> k_svB -> k_svF chain is queued by the same rule: no multi-slice source
    reaches the host, as with the always-queued chain (legacy)"""
    c = run(dict(MULTI, PPR_SV_BUDGET=str(budget), PPR_SV_RETRY_GRID=mode), monkeypatch, capfd)
    assert c["hb_multi"] == 0
    assert c["sieve_reseed_ok"] > 0


@pytest.mark.parametrize("cls", ["small", "large"])
def test_gpu_seedless(cls, monkeypatch, capfd):
    """short-row sources (a partition's first real updates) run a theta = 0 first attempt in the
    sieve; PPR_SV_SEEDLESS=0 keeps them in the range engines -- the same bits either way"""
    env = SMALL if cls == "small" else LARGE
    on = run(dict(env, PPR_SV_SEEDLESS="1"), monkeypatch, capfd, configs=ALL)
    assert on["seedless"] > 0
    assert 0 < on["seedless_done"] <= on["seedless"]
    off = run(dict(env, PPR_SV_SEEDLESS="0"), monkeypatch, capfd, configs=ALL)
    assert off["seedless"] == 0 and off["seedless_done"] == 0
    assert off["sieve_sources"] < on["sieve_sources"]


@pytest.mark.parametrize("cls", ["small", "large"])
@pytest.mark.parametrize("budget", [128, 256])
def test_gpu_seedless_overflows_seed_their_retry(cls, budget, monkeypatch, capfd):
    """with a small table the seedless attempts overflow too: their seeds are L keys of the short row
    and the table's resident keys, and the retry builds its prev table from L seeds"""
    env = SMALL if cls == "small" else LARGE
    c = run(dict(env, PPR_SV_SEEDLESS="1", PPR_SV_BUDGET=str(budget)), monkeypatch, capfd, configs=ALL)
    assert c["seedless"] > 0
    assert 0 < c["seedless_done"] <= c["seedless"]
    assert c["sieve_reseed"] > 0 and c["sieve_reseed_ok"] > 0


@pytest.mark.parametrize("off", [{"PPR_SV_RESEED": "0"}, {"PPR_SV_BUDGET": "40"}], ids=["reseed0", "budget40"])
@pytest.mark.parametrize("cls", ["small", "large"])
def test_gpu_seedless_needs_a_retry_behind_it(cls, off, monkeypatch, capfd):
    """re-seeding off, or a table budget below Lp (no seeds are written): no retry stands behind the
    launches, so short-row sources take the old path"""
    env = SMALL if cls == "small" else LARGE
    # (budget 40 is below Lp = 128 of the L = 128 and L = 96 configs; RMAT-11 runs L = 32)
    c = run(dict(env, PPR_SV_SEEDLESS="1", **off), monkeypatch, capfd, configs=ALL if "PPR_SV_RESEED" in off else ALL[1:])
    assert c["seedless"] == 0 and c["seedless_done"] == 0


def test_gpu_retry_history_is_per_job(monkeypatch, capfd):
    """GrankPlan.run twice: the overflow history starts over with every job, so both runs queue, skip
    and count the same"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(large128(), PPR_SV_MIN="0", PPR_SV_LOG="1").items():
        monkeypatch.setenv(k, v)
    scale, K, L, it = CONFIGS[1]
    g, part = graph(scale)
    o = reference(scale, K, L, it)
    plan = ppr.GrankPlan(g, K, L, 0.85, part=part, device=0)
    try:
        seen = []
        for _ in range(2):
            capfd.readouterr()
            plan.run(it, -1.0)
            r = plan.fetch()
            c = counters(capfd.readouterr().err)
            assert np.array_equal(r.lens, o["lens"])
            assert np.array_equal(r.ids, o["ids"])
            assert np.array_equal(r.scores, o["scores"])
            seen.append({k: c["log_" + k] for k in LOG_KEYS})
        print("per-run retry counters", seen)
        assert seen[0]["retry_launched"] > 0
        assert seen[0] == seen[1]
    finally:
        plan.close()
