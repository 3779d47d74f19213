"""GPU: every merge engine, forced with its knobs, on the graph families RMAT cannot produce.

The forced-engine parity tests (test_gpu_parity.py, test_gpu_sieve_*.py, test_gpu_plan_replay.py) run
on ppr.rmat: n a power of two, no repeated edge, ascending successors, cuts that tie among a handful
of keys. The graphs here (tests/graphs.py; tests/test_graph_shapes_host.py derives what each is for
from the oracle alone) are

  multigraph(1500)      repeated and unsorted successors, doubled self-loops, a node of 3,000 copies
                        of one successor, a 3,000-wide source with a full row in the LAST dense id;
                        at L = 32, at L = 96 (Lp = 128: the sieve's second-half row read of the last
                        row) and at L = 100
  multigraph(2500)      a last node of 6,000 successors, more than 1,728 of them distinct: its init
                        overflows the smallest range table when the estimates are forced 20x low
  layered(96, 8)        every updated row is cut inside a tie of 96 keys at L = 64 (more than a wave)
  layered(96, 8, half)  ... of 144 keys, two successor widths
  layered(160, 6)       ties of 160 keys at L = 128
  layered(700, 4)       669 keys outside the previous row EQUAL the sieve's bound: between the 4-wave
                        class's table (614) and the 8-wave class's (1,228)
  rmat_grafted(11, 37)  odd n, appended ids closing unsorted lists

Every case is one graph under one env set, bit-exact against the oracle (same summation mode) on
iterations_run, max_diff, lens, ids and scores, all rows. A counter's sign is asserted per case only
where the oracle implies it; test_env_reaches_its_path requires of every env with a counter of its own
that at least one of the graphs drives it.
"""
import functools
import time

import numpy as np
import pytest

import approximated_personalized_pagerank_amd as ppr
import graphs
import oracle
from test_gpu_mc import check_vs_oracle

pytestmark = pytest.mark.gpu

GRAPHS = {
    "multi1500": lambda: graphs.multigraph(1500, seed=5),
    "multi2500": lambda: graphs.multigraph(2500, seed=7, last=6000),
    "lay96": lambda: graphs.layered(96, 8),
    "lay96h": lambda: graphs.layered(96, 8, half=True),
    "lay160": lambda: graphs.layered(160, 6),
    "lay700": lambda: graphs.layered(700, 4),
    "graft11": lambda: graphs.rmat_grafted(11, 37, seed=3),
}
# (graph, K, L, iterations)
CONFIGS = [("multi1500", 16, 32, 6), ("multi1500", 32, 96, 5), ("multi1500", 32, 100, 5), ("lay96", 16, 64, 6),
           ("lay96h", 16, 64, 6), ("lay160", 32, 128, 5), ("lay700", 16, 32, 4), ("graft11", 16, 32, 5),
           ("multi2500", 16, 32, 3)]
CFG_IDS = ["%s-K%dL%d" % c[:3] for c in CONFIGS]
# every updated source of these has a full row before its last update (test_graph_shapes_host.py)
FULL_ROWS = {"multi1500", "multi2500", "lay96", "lay96h", "lay160", "lay700"}

BIG = "1000000000"
SMALL = {"PPR_SV_SMALL": BIG, "PPR_SV_MID": BIG, "PPR_TIER_MASK": "0x0"}   # every one-slice source 4 waves, redo at 8
LARGE = {"PPR_SV_SMALL": "0", "PPR_SV_MID": "0", "PPR_TIER_MASK": "0x0"}   # ... 16 waves
MID = {"PPR_SV_SMALL": "0", "PPR_SV_MID": BIG, "PPR_TIER_MASK": "0x0"}     # ... 8 waves
HBM = {"PPR_SV": "0", "PPR_XR_T": "1024", "PPR_XR_RMAX": "1", "PPR_HUB_MAX_LOGP": "1"}

# name -> (env, the counter of the env's own path or None)
BOTH = {
    "default": ({}, None),
    "mask0x0": ({"PPR_TIER_MASK": "0x0"}, None),
    "mask0x10": ({"PPR_TIER_MASK": "0x10"}, None),
    "mask0x20": ({"PPR_TIER_MASK": "0x20"}, None),
    "mask0x21": ({"PPR_TIER_MASK": "0x21"}, None),
    "mask0xf": ({"PPR_TIER_MASK": "0xf"}, None),
}
SIEVE = {  # (PPR_SV_MIN=0 in all of them)
    "sv": ({}, "sieve_sources"),
    "sv_mask0x0": ({"PPR_TIER_MASK": "0x0"}, "sieve_sources"),
    "sv_slice256": ({"PPR_SV_SLICE": "256"}, "sieve_sources"),
    "sv_small": (SMALL, "sieve_redo_dev"),
    "sv_large": (LARGE, "sieve_sources"),
    "sv_mid": (MID, "sieve_sources"),
    "sv_small_noredo": (dict(SMALL, PPR_SV_REDO="0"), "sieve_redo"),
    "sv_budget2": ({"PPR_SV_BUDGET": "2"}, "sieve_redo"),
    "sv_p2skip0": ({"PPR_SV_P2SKIP": "0"}, "sieve_sources"),
    "sv_reseed0": ({"PPR_SV_RESEED": "0"}, "sieve_sources"),
    "sv_off": ({"PPR_SV": "0"}, None),
}
SIEVE = {k: (dict(e, PPR_SV_MIN="0"), c) for k, (e, c) in SIEVE.items()}
RANGE = {
    "xr_rmax1": ({"PPR_XR_RMAX": "1"}, None),
    "xr_dscale5": ({"PPR_XR_DSCALE": "5"}, "xr_redo"),
    "xr_t1024_fill20": ({"PPR_XR_T": "1024", "PPR_XR_FILL": "20"}, None),
    "xr_listcap0": ({"PPR_XR_LISTCAP": "0"}, None),
    "wave_split0": ({"PPR_WAVE_SPLIT": "0"}, None),
    "wave_split256_cap1": ({"PPR_WAVE_SPLIT": "256", "PPR_WAVE_CAP": "1"}, None),
    "xm": ({"PPR_XM": "1", "PPR_SV": "0"}, None),
    "wave_tdiv3": ({"PPR_WAVE_TDIV": "3"}, "wave_redo"),
    "hbm": (HBM, "hbm_table"),
    "hbm_cap1": (dict(HBM, PPR_XG_CAP="1"), "hbm_table"),
}
HUB = {  # chain mode: the hub pipeline
    "hub_seg0": ({"PPR_HUB_SEG": "0"}, "hubs"),
    "hub_seg1_b64": ({"PPR_HUB_SEG": "1", "PPR_SEG_BUCKET": "64"}, "hubs"),
    "hub_range0": ({"PPR_HUB_RANGE": "0"}, "hubs"),
    "hub_range3_b64": ({"PPR_HUB_RANGE": "3", "PPR_HUB_BUCKET": "64"}, "hubs"),
    "hot64": ({"PPR_HOT_N": "64", "PPR_HOT_AT": "0"}, "hubs"),
    "spec1": ({"PPR_SPEC": "1.0", "PPR_SPEC_FROM": "1"}, "spec_redo"),
    "lds_rank0": ({"PPR_LDS_RANK": "0"}, "hubs"),
    "hub_slice64": ({"PPR_HUB_SLICE": "64", "PPR_TIER_MASK": "0x21"}, "hubs"),
    "wave_split_chain256": ({"PPR_WAVE_SPLIT_CHAIN": "256"}, None),
}
EXACT_ENVS = {**BOTH, **SIEVE, **RANGE}
CHAIN_ENVS = {**BOTH, **HUB}
ENVS = {"exact": EXACT_ENVS, "chain": CHAIN_ENVS}
KNOBS = sorted({k for envs in ENVS.values() for e, _ in envs.values() for k in e} |
               {"PPR_SV_MIN", "PPR_SV_REDO_LARGE", "PPR_SV_RESEED_BUDGET", "PPR_SV_RETRY_GRID", "PPR_SV_SEEDLESS",
                "PPR_WAVE_BY_D", "PPR_REPLAY", "PPR_SV_LOG", "PPR_HUB_BUDGET", "PPR_XR_BUDGET", "PPR_WHATIF",
                "PPR_MC_SUM", "PPR_DIAG"})

_TABLE = {}  # (config id, mode, env name) -> counters of the case, once it passed


@functools.lru_cache(maxsize=None)
def graph(name):
    g = ppr.Csr(*GRAPHS[name]())
    return g, g.partitions()


@functools.lru_cache(maxsize=None)
def reference(cfg, mode, it=None):
    name, K, L, its = cfg
    g, part = graph(name)
    with oracle.sum_mode(mode):
        o = oracle.grank(g.row_ptr, g.col, part, K, L, its if it is None else it, 0.85, -1.0)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def setenv(env, mode, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PPR_TIMING", "1")
    monkeypatch.setenv("PPR_SUM", mode)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def counters(err):
    c = {"sieve_sources": 0, "sieve_redo": 0, "sieve_redo_dev": 0, "sieve_reseed": 0, "sieve_reseed_ok": 0,
         "xr_redo": 0, "wave_redo": 0, "hbm_table": 0, "spec_redo": 0, "hubs": 0, "recorded": 0, "replayed": 0,
         "dropped": 0, "len_changes": 0}
    for ln in err.splitlines():
        f = ln.split()
        if ln.startswith("ppr_timing sieve_sources") or ln.startswith("ppr_timing replay"):
            for i in range(1 if f[1] == "sieve_sources" else 2, len(f) - 1, 2):
                c[f[i]] += int(f[i + 1])
        elif ln.startswith("ppr_timing hub_planning"):
            c["hubs"] += int(f[f.index("hubs") + 1])
        else:
            for k in ("xr_redo", "wave_redo", "hbm_table", "spec_redo"):
                if ln.startswith("ppr_timing %s_sources" % k):
                    c[k] += int(f[2])
    return c


def first_difference(g, r, o):
    """where a mismatch starts: the first differing source, its successors and distinct successors"""
    for what, a, b in (("lens", r.lens, o["lens"]), ("ids", r.ids, o["ids"]), ("scores", r.scores, o["scores"])):
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            v = int(bad[0])
            s = g.col[g.row_ptr[v]:g.row_ptr[v + 1]]
            return "%s differ in %d rows, first source %d (n %d): %d successors, %d distinct" % (
                what, len(bad), v, g.n, len(s), len(np.unique(s)))
    return ""


def run_case(ci, mode, ename, monkeypatch, capfd):
    key = (CFG_IDS[ci], mode, ename)
    if key in _TABLE:
        return _TABLE[key]
    cfg = CONFIGS[ci]
    name, K, L, it = cfg
    env = ENVS[mode][ename][0]
    g, part = graph(name)
    o = reference(cfg, mode)
    setenv(env, mode, monkeypatch)
    capfd.readouterr()
    t0 = time.perf_counter()
    r = ppr.grank_csr(g, K, L, it, 0.85, -1.0, part=part, device=0)
    dt = time.perf_counter() - t0
    err = capfd.readouterr().err
    c = counters(err)
    print("shape_case %s %s %s %.3f s %s" % (key[0], mode, ename, dt, {k: v for k, v in c.items() if v}))
    print("\n".join(ln for ln in err.splitlines() if ln.startswith("ppr_timing") and "_s " not in ln))
    assert r.iterations_run == o["iterations_run"]
    why = first_difference(g, r, o)
    assert np.array_equal(r.max_diff, o["max_diff"]), why
    assert np.array_equal(r.lens, o["lens"]), why
    assert np.array_equal(r.ids, o["ids"]), why
    assert np.array_equal(r.scores, o["scores"]), why
    # counter signs the oracle implies
    sieve_on = mode == "exact" and env.get("PPR_SV_MIN") == "0" and env.get("PPR_SV") != "0"
    if mode == "exact" and env.get("PPR_SV") == "0":
        assert c["sieve_sources"] == 0
    if sieve_on and env.get("PPR_TIER_MASK") == "0x0" and name in FULL_ROWS:
        assert c["sieve_sources"] > 0  # no wave tier: every source with a full row is offered to the sieve
    if name == "lay700" and ename == "sv_small":
        # 669 keys must enter the pass-2 table: past the 4-wave class's budget of 614, within the redo's
        # 1,228. (A table flags its overflow when a wave brings passing keys after the fill has passed
        # the budget; each of the 669 is a candidate exactly once, so a source overflows when one of its
        # four waves flushes its last keys late: measured 850-897 of the 5,600 sieved sources.)
        assert c["sieve_redo_dev"] > 0
        assert c["sieve_redo"] == 0
    if name == "lay700" and ename == "sv_small_noredo":
        assert c["sieve_redo"] > 0
    _TABLE[key] = c
    return c


CASES = [(ci, mode, e) for mode in ("exact", "chain") for e in ENVS[mode] for ci in range(len(CONFIGS))]


@pytest.mark.parametrize("ci,mode,ename", CASES, ids=["%s-%s-%s" % (CFG_IDS[ci], m, e) for ci, m, e in CASES])
def test_gpu_graph_shape_bit_exact(ci, mode, ename, monkeypatch, capfd):
    run_case(ci, mode, ename, monkeypatch, capfd)


PATHS = [(mode, e) for mode in ("exact", "chain") for e, (_, ctr) in ENVS[mode].items() if ctr]


@pytest.mark.parametrize("mode,ename", PATHS, ids=["%s-%s" % p for p in PATHS])
def test_env_reaches_its_path(mode, ename, monkeypatch, capfd):
    """at least one of the graphs drives the path the env is there to force (cases that already ran
    are read from the table; any other runs here)"""
    ctr = ENVS[mode][ename][1]
    per = {CFG_IDS[ci]: run_case(ci, mode, ename, monkeypatch, capfd)[ctr] for ci in range(len(CONFIGS))}
    print("shape_path %s %s %s %s" % (mode, ename, ctr, per))
    assert sum(per.values()) > 0
    if ename.startswith("sv") and ename != "sv_off":
        assert sum(run_case(ci, mode, ename, monkeypatch, capfd)["sieve_sources"] for ci in range(len(CONFIGS))) > 0


def test_gpu_replay_on_ties(monkeypatch, capfd):
    """layered(96, 8), default knobs, 12 iterations: an update replays exactly when the two updates
    before it changed no row length, and the device counted the changed rows as the oracle's rows say
    (the rule of test_gpu_plan_replay.expected, from the oracle's row lengths alone)"""
    cfg = ("lay96", 16, 64, 12)
    name, K, L, it = cfg
    g, part = graph(name)
    lens = [oracle.grank(g.row_ptr, g.col, part, K, L, k, 0.85, -1.0, want_slab=True)["slab_lens"].copy()
            for k in range(it + 1)]
    chg = [int(np.count_nonzero(lens[u + 1] != lens[u])) for u in range(it)]
    want = sum(1 for u in range(2, it) if chg[u - 2] == 0 and chg[u - 1] == 0)
    assert want > 0
    setenv({}, "exact", monkeypatch)
    capfd.readouterr()
    r = ppr.grank_csr(g, K, L, it, 0.85, -1.0, part=part, device=0)
    c = counters(capfd.readouterr().err)
    print("shape_replay", chg, c)
    o = reference(cfg, "exact")
    assert r.iterations_run == o["iterations_run"] and np.array_equal(r.max_diff, o["max_diff"])
    assert np.array_equal(r.lens, o["lens"]) and np.array_equal(r.ids, o["ids"]) and np.array_equal(r.scores, o["scores"])
    assert c["replayed"] == want
    assert c["len_changes"] == sum(chg)


@pytest.mark.parametrize("mask", [None, "0x20"], ids=["default", "mask0x20"])
@pytest.mark.parametrize("name", ["multi1500", "lay96"])
def test_gpu_mc_graph_shapes(name, mask, monkeypatch):
    """the MC walks and combine on repeated successors and on mass ties equal the MC oracle"""
    setenv({} if mask is None else {"PPR_TIER_MASK": mask}, "exact", monkeypatch)
    monkeypatch.delenv("PPR_SUM")
    g, _ = graph(name)
    check_vs_oracle(g, 16, 64, 100, 0.85)
