"""Host: what the GPU cases of tests/test_gpu_graph_shapes.py depend on, from the oracle alone.

The generators of tests/graphs.py exist to put inputs in front of the merge engines that RMAT never
produces: repeated successors, cuts inside ties wider than a wave, a tie that lands between two sieve
table budgets, a wide source in the last dense id. Each condition is derived here from the CPU oracle
(full merged values: the oracle's slab padded to width n and one oracle.step at L = n, so nothing is
cut), so an edit to a generator cannot quietly remove what a GPU case is there for.
"""
import functools

import numpy as np

import approximated_personalized_pagerank_amd as ppr
import graphs
import oracle
from test_oracle_xsum import _exact_step

D = 0.85
SV_SMALL_BUDGET, SV_MID_BUDGET = 614, 1228  # csrc/merge_sv.h sv_geom(11, 4).budget, sv_geom(12, 8).budget


def partitions(rp, col):
    return ppr.Csr(rp, col).partitions()


def full_update(rp, col, L, u, pick=slice(None)):
    """update u (0-based: it merges partition u & 1 from the state after u iterations) without its
    cut: (sources, ids, values, counts) with every merged key of a source by (value desc, id asc), and
    the width-L slab the update read"""
    n = len(rp) - 1
    part = partitions(rp, col)
    with oracle.sum_mode("exact"):
        st = oracle.grank(rp, col, part, L, L, u, D, -1.0, want_slab=True)
        ids = np.full((n, n), -1, dtype=np.int32)
        sc = np.zeros((n, n), dtype=np.float64)
        ids[:, :L], sc[:, :L] = st["slab_ids"], st["slab_scores"]
        act = np.nonzero((part == (u & 1)) & (np.diff(rp) > 0))[0].astype(np.int32)[pick]
        fi, fs, fl, _ = oracle.step(rp, col, n, D, (ids, sc, st["slab_lens"]), act)
    return act, fi, fs, fl, st


def tie_stats(rp, col, L, u):
    """(updated rows, rows the cut truncates, rows whose cut falls inside a tie, most keys at a cut value)"""
    act, _, fs, fl, _ = full_update(rp, col, L, u)
    trunc = tied = most = 0
    for r in range(len(act)):
        if fl[r] > L:
            v = fs[r, :fl[r]]
            trunc += 1
            tied += v[L] == v[L - 1]
            most = max(most, int((v == v[L - 1]).sum()))
    return len(act), trunc, tied, most


def test_oracle_exact_step_matches_rationals_on_multigraph():
    """tests/test_oracle_xsum.py::test_exact_step_matches_definition on a multigraph: a repeated
    successor contributes once per list entry and deg counts entries"""
    rp, col = graphs.multigraph(300, seed=3, hub=700)
    assert len(col) - sum(len(np.unique(col[rp[v]:rp[v + 1]])) for v in range(300)) > 1000  # repeated entries
    part = partitions(rp, col)
    L = 32
    with oracle.sum_mode("exact"):
        st = oracle.grank(rp, col, part, L, L, 3, D, -1.0, want_slab=True)
        slab = (st["slab_ids"], st["slab_scores"], st["slab_lens"])
        act = np.nonzero((part == 1) & (np.diff(rp) > 0))[0].astype(np.int32)  # iteration 3 updates partition 1
        nid, nsc, nln, _ = oracle.step(rp, col, L, D, slab, act)
    checked = 0
    for r, v in enumerate(act):
        want = _exact_step(rp, col, L, D, slab[0], slab[1], slab[2], int(v))
        got = dict(zip(nid[r, :nln[r]].tolist(), nsc[r, :nln[r]].tolist()))
        for k, x in got.items():
            assert x == want[k], (v, k)
        cut = min(got.values())
        assert all(x <= cut for k, x in want.items() if k not in got)
        assert len(got) == min(L, len(want))
        checked += len(got)
    assert checked > 500
    assert 0 in act or 299 in act  # a hub row among them


def test_from_dict_keeps_duplicates_and_order():
    d = {"a": ["b", "b", "a", "c", "b"], "b": ["c", "a", "c"], "c": ["c", "c"]}
    g = ppr.Csr.from_dict(d)
    assert g.row_ptr.tolist() == [0, 5, 8, 10]
    assert g.col.tolist() == [1, 1, 0, 2, 1, 2, 0, 2, 2, 2]
    rp, col = graphs.multigraph(50, seed=1, hub=20)
    lists = {v: col[rp[v]:rp[v + 1]].tolist() for v in range(50)}
    g = ppr.Csr.from_dict(lists)
    assert np.array_equal(g.row_ptr, rp) and np.array_equal(g.col, col)
    assert lists[0] == [1] * 20 + [2, 3, 2] and lists[7].count(7) >= 2
    assert any(s != sorted(s) for s in lists.values())


def test_layered_96_cuts_every_row_inside_a_tie_wider_than_a_wave():
    for half in (False, True):
        rows, trunc, tied, most = tie_stats(*graphs.layered(96, 8, half=half), 64, 5)
        print("layered(96, 8, half=%s) L64 update 5:" % half, rows, trunc, tied, most)
        assert trunc == rows and tied == rows
        assert most > 64


def test_layered_160_ties_at_l128():
    rows, trunc, tied, most = tie_stats(*graphs.layered(160, 6), 128, 4)
    print("layered(160, 6) L128 update 4:", rows, trunc, tied, most)
    assert 2 * tied >= rows
    assert most > 128


def test_layered_700_tie_lands_between_the_small_and_mid_sieve_budgets():
    """keys outside the previous row that reach theta (the smallest new total of the previous row's
    keys) must all enter the sieve's pass-2 table: more than the 4-wave class holds, fewer than the
    8-wave class, and every one of them EQUALS theta"""
    rp, col = graphs.layered(700, 4)
    L = 32
    for u in range(4):
        act, fi, fs, fl, st = full_update(rp, col, L, u, pick=slice(None, None, 97))
        assert len(act) >= 10
        for r, v in enumerate(act):
            assert st["slab_lens"][v] == L  # a full row: the sieve takes the source
            prev = set(st["slab_ids"][v, :L].tolist())
            tot = dict(zip(fi[r, :fl[r]].tolist(), fs[r, :fl[r]].tolist()))
            theta = min(tot[k] for k in prev)
            outside = [x for k, x in tot.items() if k not in prev and x >= theta]
            assert SV_SMALL_BUDGET < len(outside) < SV_MID_BUDGET, (u, v, len(outside))
            assert all(x == theta for x in outside)
            assert int((fs[r, :fl[r]] == fs[r, L - 1]).sum()) > 64 * 4  # the cut's tie: more than the class's lanes


@functools.lru_cache(maxsize=None)
def _multigraph_1500():
    return graphs.multigraph(1500, seed=5)


def test_multigraph_last_dense_id_is_a_wide_source_with_a_full_row():
    rp, col = _multigraph_1500()
    n = len(rp) - 1
    part = partitions(rp, col)
    succ = col[rp[n - 1]:rp[n]]
    assert len(succ) == 3000 and rp[1] == 3003 and len(np.unique(col[:3003])) == 3
    for L in (32, 64, 96, 100):
        lens = oracle.grank(rp, col, part, L, L, 0, D, -1.0, want_slab=True)["slab_lens"]
        assert lens[n - 1] == L
        assert int(lens[succ].sum()) > 64 * L
        assert int(lens[col[:3003]].sum()) > 64 * L  # node 0: candidates far above its distinct keys


def test_multigraph_2500_init_must_overflow_a_range_table_planned_20x_low():
    """PPR_XR_DSCALE=5 plans a source's tables for a twentieth of its expected distinct keys. The init of
    the last node (6,000 successors, no earlier count: 60 % of the candidates + 64 expected) is then
    planned as one range in the smallest table class -- 2,048 slots, stopped at min(85 %, slots - 5
    waves of lanes) = 1,728 keys (grank.hip run_xhubs estimate, xr_classes, xr_queue) -- and has more
    distinct keys than that: the table overflows, the source is redone. No graph of at most 1,728
    nodes can do this."""
    rp, col = graphs.multigraph(2500, seed=7, last=6000)
    n = len(rp) - 1
    succ = col[rp[n - 1]:rp[n]]
    c = len(succ)
    assert c == 6000
    planned = min(c, c * 3 // 5 + 64) * 5 // 100
    assert planned <= 2048 * 85 // 100  # one range of the smallest class
    assert len(set(succ.tolist()) | {n - 1}) > min(2048 * 85 // 100, 2048 - 4 * 64 - 64)
    lens = oracle.grank(rp, col, partitions(rp, col), 32, 32, 0, D, -1.0, want_slab=True)["slab_lens"]
    assert lens[n - 1] == 32 and int(lens[succ].sum()) > 64 * 32


def test_rmat_grafted_has_odd_n_and_unsorted_lists():
    rp, col = graphs.rmat_grafted(11, 37, seed=3)
    n = len(rp) - 1
    assert n == 2048 + 37 and n % 2 == 1
    assert all(rp[v + 1] > rp[v] for v in range(2048, n))
    assert np.count_nonzero(col >= 2048) >= 37
