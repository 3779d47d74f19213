"""GPU: recorded merge plans replayed while no basket length changes (replay_rule.h).

An exact-sum update plans from row lengths only, so the plan a partition recorded two updates
earlier is replayed -- no k_classify, no gather, no host planning, no descriptor upload -- while the
device count of row-length changes stands still. Which engine merges a source never changes a bit
of its row: every run here is bit-exact against the oracle's exact sum on max_diff, lens, ids and
scores. The `ppr_timing replay` line (recorded / replayed / dropped / len_changes, summed over the
plans of a case) says what ran, and the expected figures come from the oracle alone: its row
lengths after the init and after every update give the rows whose length an update changed, and
update it >= 2 must replay exactly when updates it - 2 and it - 1 changed none.
"""
import functools

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
import oracle

pytestmark = pytest.mark.gpu

# 12 iterations: the lengths stop changing with updates to spare (RMAT-11 L=32 after its 4th update,
# RMAT-12 L=128 after its 5th). Neither graph can produce a partitioned source: a source has at most
# 2,048 / 4,096 distinct keys, below four range tables.
CONFIGS = [(11, 16, 32, 12), (12, 32, 128, 12)]
PATH = ("path", 16, 32, 12)  # v -> v + 1, 4,096 nodes: a node's reachable set grows for about L updates

LARGE = {"PPR_SV_SMALL": "0", "PPR_SV_MID": "0", "PPR_TIER_MASK": "0x0"}  # every one-slice source 16 waves
SMALL = {"PPR_SV_SMALL": "1000000000", "PPR_SV_MID": "1000000000", "PPR_TIER_MASK": "0x0"}  # 4 waves, redo at 8
KNOBS = ["PPR_SV_SMALL", "PPR_SV_MID", "PPR_TIER_MASK", "PPR_SV_REDO_LARGE", "PPR_SV_SLICE", "PPR_SV_BUDGET",
         "PPR_SV_RESEED", "PPR_SV_RESEED_BUDGET", "PPR_SV_RETRY_GRID", "PPR_SV_SEEDLESS", "PPR_SV", "PPR_WAVE_TDIV",
         "PPR_WAVE_BY_D", "PPR_HOT_N", "PPR_REPLAY", "PPR_SV_LOG"]
REPLAY_KEYS = ["recorded", "replayed", "dropped", "len_changes"]
RETRY_KEYS = ["launched", "skipped", "past_grid", "seedless", "seedless_done"]
LOG_KEYS = ["retry_launched", "retry_skipped", "past_grid", "seedless", "seedless_done"]


@functools.lru_cache(maxsize=None)
def graph(scale):
    if scale == "path":
        n = 4096
        g = ppr.Csr(np.concatenate([np.arange(n, dtype=np.int64), [n - 1]]), np.arange(1, n, dtype=np.int32))
    else:
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


@functools.lru_cache(maxsize=None)
def expected(scale, K, L, it):
    """(updates that must replay, rows whose length the updates changed) from the oracle's row lengths
    after the init (0 iterations) and after each of the `it` updates"""
    g, part = graph(scale)
    lens = [oracle.grank(g.row_ptr, g.col, part, K, L, k, 0.85, -1.0, want_slab=True)["slab_lens"].copy()
            for k in range(it + 1)]
    chg = [int(np.count_nonzero(lens[u + 1] != lens[u])) for u in range(it)]
    replayed = sum(1 for u in range(2, it) if chg[u - 2] == 0 and chg[u - 1] == 0)
    return replayed, sum(chg), tuple(chg)


def counters(err):
    c = {"sieve_sources": 0, "sieve_redo": 0, "sieve_redo_dev": 0, "sieve_reseed": 0, "sieve_reseed_ok": 0,
         "wave_redo": 0}
    c.update({k: 0 for k in REPLAY_KEYS + RETRY_KEYS})
    c.update({"log_" + k: 0 for k in LOG_KEYS})
    for ln in err.splitlines():
        f = ln.split()
        if (ln.startswith("ppr_timing sieve_sources") or ln.startswith("ppr_timing sieve_retry")
                or ln.startswith("ppr_timing replay")):
            for i in range(1 if f[1] == "sieve_sources" else 2, len(f) - 1, 2):
                c[f[i]] += int(f[i + 1])
        elif ln.startswith("ppr_timing wave_redo_sources"):
            c["wave_redo"] += int(f[2])
        elif ln.startswith("ppr_sv_log"):
            for k in LOG_KEYS:
                c["log_" + k] += int(f[f.index(k) + 1])
    return c


def setenv(env, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PPR_SV_MIN", "0")
    monkeypatch.setenv("PPR_TIMING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check(r, o):
    assert np.array_equal(r.lens, o["lens"])
    assert np.array_equal(r.ids, o["ids"])
    assert np.array_equal(r.scores, o["scores"])


def run(env, monkeypatch, capfd, configs=CONFIGS):
    """the configs under `env`, each bit-exact against the oracle; the summed counters"""
    setenv(env, monkeypatch)
    capfd.readouterr()
    for scale, K, L, it in configs:
        g, part = graph(scale)
        r = ppr.grank_csr(g, K, L, it, 0.85, -1.0, part=part, device=0)
        o = reference(scale, K, L, it)
        assert np.array_equal(r.max_diff, o["max_diff"])
        check(r, o)
    c = counters(capfd.readouterr().err)
    print("replay counters", env, c)
    return c


def test_gpu_replay_default_knobs(monkeypatch, capfd):
    """every update the rule allows replays, no other does, and the device counted the rows whose
    length changed exactly as the oracle's rows say"""
    for cfg in CONFIGS:
        want_replayed, want_changes, chg = expected(*cfg)
        print("oracle length changes per update", cfg, chg)
        c = run({}, monkeypatch, capfd, configs=[cfg])
        assert want_replayed > 0
        assert c["replayed"] == want_replayed
        assert c["len_changes"] == want_changes
        assert c["recorded"] == cfg[3] - want_replayed  # every other update recorded its plan


def test_gpu_replay_on_and_off(monkeypatch, capfd):
    """PPR_REPLAY=0 is the path without recorded plans: the same results (run() checks both against
    the oracle), and the algorithmic bytes -- the device's and the kernel groups' -- to the byte"""
    seen = {}
    for mode in ("1", "0"):
        setenv({"PPR_REPLAY": mode}, monkeypatch)
        capfd.readouterr()
        figs = []
        for scale, K, L, it in CONFIGS:
            g, part = graph(scale)
            plan = ppr.GrankPlan(g, K, L, 0.85, part=part, device=0, stats=True)
            try:
                st = plan.run(it, -1.0)
                check(plan.fetch(), reference(scale, K, L, it))
                ks = plan.kernel_stats()
                figs.append((int(st.algo_bytes), int(st.candidates), [ks[k]["algo_bytes"] for k in plan.KERNEL_GROUPS],
                             [ks[k]["launches"] for k in plan.KERNEL_GROUPS]))
            finally:
                plan.close()
        seen[mode] = (figs, counters(capfd.readouterr().err))
    print("replay on / off", seen)
    assert seen["1"][1]["replayed"] > 0
    assert seen["0"][1]["replayed"] == 0 and seen["0"][1]["recorded"] == 0
    assert seen["1"][0] == seen["0"][0]
    assert seen["1"][1]["len_changes"] == seen["0"][1]["len_changes"]


@pytest.mark.parametrize("env", [LARGE, SMALL, {"PPR_SV_SLICE": "256"}, {"PPR_SV": "0"}],
                         ids=["large", "small", "multi_slice", "range_only"])
def test_gpu_replay_each_engine(env, monkeypatch, capfd):
    """one engine at a time takes the wide sources of the replayed updates"""
    c = run(env, monkeypatch, capfd, configs=CONFIGS[1:])
    assert c["replayed"] == expected(*CONFIGS[1])[0] > 0
    if env.get("PPR_SV") == "0":
        assert c["sieve_sources"] == 0
    else:
        assert c["sieve_sources"] > 0


@pytest.mark.parametrize("env", [dict(LARGE, PPR_SV_BUDGET="128"), {"PPR_WAVE_TDIV": "2"}], ids=["sieve", "wave"])
def test_gpu_replay_overflows(env, monkeypatch, capfd):
    """overflows during replayed updates take the usual way: the device retries from this update's
    grid rule, and hand-backs and wave-tier redos are planned afresh on the host"""
    c = run(dict(env, PPR_SV_LOG="1"), monkeypatch, capfd)
    assert c["replayed"] == sum(expected(*cfg)[0] for cfg in CONFIGS)
    assert c["sieve_reseed"] > 0 or c["wave_redo"] > 0
    for k, lk in zip(RETRY_KEYS, LOG_KEYS):
        assert c[k] == c["log_" + lk]


def test_gpu_replay_lengths_keep_changing(monkeypatch, capfd):
    """a directed path: every update lengthens some row, so no update may replay"""
    want_replayed, want_changes, chg = expected(*PATH)
    assert want_replayed == 0 and min(chg) > 0
    c = run({}, monkeypatch, capfd, configs=[PATH])
    assert c["replayed"] == 0
    assert c["len_changes"] == want_changes


def test_gpu_replay_is_per_job(monkeypatch, capfd):
    """GrankPlan.run twice: a repeated run is a cold call, no plan of the first run survives its init"""
    setenv({}, monkeypatch)
    scale, K, L, it = CONFIGS[1]
    g, part = graph(scale)
    o = reference(scale, K, L, it)
    seen = []
    for runs in (1, 2):
        capfd.readouterr()
        plan = ppr.GrankPlan(g, K, L, 0.85, part=part, device=0)
        try:
            for _ in range(runs):
                plan.run(it, -1.0)
                check(plan.fetch(), o)
        finally:
            plan.close()
        seen.append(counters(capfd.readouterr().err))
    print("one run / two runs", seen)
    assert seen[0]["replayed"] == expected(scale, K, L, it)[0]
    for k in ("recorded", "replayed", "len_changes"):
        assert seen[1][k] == 2 * seen[0][k]


def test_gpu_replay_public_iterate(monkeypatch, capfd):
    """the second replay-eligible update issued as two half ranges through ppr_grank_plan_iterate: a
    plan covers one list range, so neither half replays (nor does the next update of that list, whose
    record is a half's), and the result is the same"""
    setenv({}, monkeypatch)
    scale, K, L, it = CONFIGS[0]
    g, part = graph(scale)
    o = reference(scale, K, L, it)
    chg = expected(scale, K, L, it)[2]
    ok = [u for u in range(2, it) if chg[u - 2] == 0 and chg[u - 1] == 0]
    assert len(ok) >= 2
    split = ok[1]
    capfd.readouterr()
    plan = ppr.GrankPlan(g, K, L, 0.85, part=part, device=0)
    try:
        plan.init()
        md = []
        for u in range(it):
            n = plan.active_count(u)
            if u == split:
                plan.iterate(u, 0, n // 2)
                plan.iterate(u, n // 2, n)
            else:
                plan.iterate(u, 0, n)
            md.append(plan.read_maxdiff(u))
        plan.finish(it)
        r = plan.fetch()
    finally:
        plan.close()
    c = counters(capfd.readouterr().err)
    print("public iterate", c, "split", split)
    assert np.array_equal(np.array(md), o["max_diff"])
    check(r, o)
    assert c["replayed"] == len(ok) - 1 - (1 if split + 2 in ok else 0)
