"""Shared helpers for the parity tests (fixtures, tie-aware comparisons)."""
from __future__ import annotations

import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixtures whose reference run never truncates a basket at a tie: bit-exact targets (P2)
EXACT = [
    "g1_ring100", "g1_ring100_multi", "g2_rmat8_full", "g5_noedges10", "g5_single", "g5_single_loop",
    "g5_two_linked", "g5_ring6", "g5_ring6_k3l4", "g5_star", "g5_star_loop", "g5_ring100_k10_l10",
    "g5_ring100_k10_l20", "g5_ring100_full", "g5_instar_full", "g5_instar_loop_full",
    "g5_instar_all_full", "g5_random5000_full", "g5_complete_full", "g6_multigraph_full",
]
# truncating runs: statistical parity (P3/P4, tests/test_parity_p34.py), top-K Jaccard thresholds
# just under the reference-vs-relabelled-reference agreement (fixture field self_jaccard)
STAT = {
    "g3_rmat12_k16_l32": 0.945,   # the reference vs itself relabelled: 0.958-0.963
    "g3_rmat14_k32_l64": 0.975,   # ... 0.986-0.987
    "g3_rmat14_k64_l128": 0.915,  # ... 0.921-0.934
    "g4_eat_k50_l100": 0.99,
}


def load(name: str):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    K, L, it, d, tol = z["params"]
    return dict(z=z, K=int(K), L=int(L), iters=int(it), damping=float(d), tol=float(tol),
                rp=z["rp"], col=z["col"], part=z["part"])


def all_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")))


def ref_rows(f):
    z = f["z"]
    cnt = np.minimum(z["cnt"], f["K"])
    return z["ids"], z["scores"], cnt, (z["sample"] if "sample" in z else None)


def jaccard_rows(ai, al, bi, bl):
    js = np.empty(len(al))
    for v in range(len(al)):
        a = set(ai[v, : al[v]].tolist())
        b = set(bi[v, : bl[v]].tolist())
        js[v] = 1.0 if not (a or b) else len(a & b) / len(a | b)
    return js


def tie_aware_recall(ai, asc, al, bi, bsc, bl, tol=1e-12):
    """fraction of b's entries whose score is matched by some a entry within tol (ties allowed)"""
    hit = tot = 0
    for v in range(len(al)):
        sa = np.sort(asc[v, : al[v]])
        for s in bsc[v, : bl[v]]:
            tot += 1
            j = np.searchsorted(sa, s - tol)
            hit += j < len(sa) and abs(sa[j] - s) <= tol * max(1.0, abs(s))
    return hit / max(tot, 1)


# exact-sum mode vs the reference's fma chain: every score agrees to this relative tolerance
# (the exact sum of the rounded products, rounded once, against a chain that rounds
# after every add -- a few ulps apart; 1e-12 leaves a wide margin)
XSUM_RTOL = 1e-12


def rows_close(ai, asc, al, bi, bsc, bl, rtol=XSUM_RTOL):
    """row by row: same lengths, every key present in both with scores within rtol, and a key in
    only one row only where its score is within rtol of that row's K-th (a near-tie at the cut
    that the two summation orders may break differently). Returns the number of such swaps."""
    swaps = 0
    assert np.array_equal(al, bl)
    for v in range(len(al)):
        n = int(al[v])
        a = dict(zip(ai[v, :n].tolist(), asc[v, :n].tolist()))
        b = dict(zip(bi[v, :n].tolist(), bsc[v, :n].tolist()))
        for k in a.keys() & b.keys():
            assert abs(a[k] - b[k]) <= rtol * abs(b[k]), (v, k, a[k], b[k])
        for side, other in ((a, b), (b, a)):
            for k in side.keys() - other.keys():
                lo = min(other.values())
                assert abs(side[k] - lo) <= rtol * abs(lo), (v, k, side[k], lo)
                swaps += 1
    return swaps
