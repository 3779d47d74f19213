"""Throughput of the node-pair scores (GrankPlan.pairs) on the flagship plan.

Setup: RMAT-22, K64 / L128, after bench.py's 30-iteration job. Workloads:
  random_pairs     2^20 uniformly drawn (u, v), grouped by u, lookup outputs only: once the probes
                   alone (fwd, bwd, hit) and once with rank and both row lengths
  rerank_1024      4096 sources x 1024 uniformly drawn candidates, every output
  own_row          4096 sources, each against the keys of its own row, every output
Protocol: warm-up calls, then >= 10 timed repetitions of the raw C call into arrays allocated once;
per repetition the device_ms (HIP events around the kernels, uploads and downloads excluded) and the
host clock around the whole call. Reported: median, minimum and maximum, pairs/s from the device time
and from the wall time, algo_bytes / device_ms against the 8 TB/s HBM peak, tier counts, the library
digest. The overlap workloads are repeated under the knobs that move groups between the tiers and
switch the LDS search, alternating with the default in the same process.
For comparison, the path a user has without the feature: fetch_slab once (timed), then per pair a
dictionary lookup and a numpy intersection of the two rows on a sample of each workload, scaled to the
workload's size, with the results compared for equality.
Writes profiles/pairs_rmat22_k64_l128.json (or --out); nothing in it is asserted anywhere.

    python tools/pairs_bench.py [--scale 22] [--reps 10] [--no-baseline]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import approximated_personalized_pagerank_amd as ppr  # noqa: E402
from approximated_personalized_pagerank_amd import _lib, build as _build  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
OUTS = ("fwd", "bwd", "hit", "rank", "common", "dot", "slen", "clen")
DT = dict(fwd=np.float64, bwd=np.float64, hit=np.uint8, rank=np.int32, common=np.int32, dot=np.float64, slen=np.int32,
          clen=np.int32)
KNOBS = ("PPR_PR_WAVE_MAX", "PPR_PR_SPLIT", "PPR_PR_CHUNK", "PPR_PR_SEARCH")


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "n": len(xs)}


class Call:
    """one workload's raw call: the arrays are allocated once"""

    def __init__(self, plan, gptr, src, cands, outs):
        self.plan, self.gptr, self.src, self.cands = plan, gptr, src, cands
        self.o = {k: (np.zeros(max(len(src) if k == "slen" else len(cands), 1), dtype=DT[k]) if k in outs else None) for k in OUTS}
        self.st = _lib.PprPairsStats()

    def __call__(self):
        t0 = time.perf_counter()
        rc = _lib.lib().ppr_grank_plan_pairs(self.plan._p, self.plan.iterations_run, len(self.src), _lib.ptr(self.gptr),
                                             _lib.ptr(self.src), _lib.ptr(self.cands), 0, *(_lib.ptr(self.o[k]) for k in OUTS),
                                             ctypes.byref(self.st))
        wall = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, "plan_pairs")
        return float(self.st.device_ms), wall


def report(call, dev, wall):
    st, P = call.st, len(call.cands)
    d, w = spread(dev), spread(wall)
    return {"pairs": P, "groups": len(call.src), "outputs": [k for k in OUTS if call.o[k] is not None],
            "device_ms": d, "wall_ms": w, "M_pairs_per_s_device": P / 1e6 / (d["median"] / 1e3),
            "M_pairs_per_s_wall": P / 1e6 / (w["median"] / 1e3), "algo_bytes": int(st.algo_bytes),
            "share_of_hbm_peak": int(st.algo_bytes) / (d["median"] / 1e3) / HBM_PEAK, "entries_read": int(st.entries_read),
            "class": "overlap" if st.overlap_pairs else "lookup",
            "tiers": {"wave": int(st.wave_groups), "workgroup": int(st.wg_groups), "split": int(st.split_groups)},
            "chunks": int(st.chunks)}


def measure(call, warmup, reps, variants=()):
    """the default and every knob variant, alternating within each repetition"""
    sets = [("default", {})] + list(variants)
    dev = {n: [] for n, _ in sets}
    wall = {n: [] for n, _ in sets}
    stats = {}
    for r in range(warmup + reps):
        for name, env in sets:
            for k, v in env.items():
                os.environ[k] = str(v)
            d, w = call()
            for k in env:
                del os.environ[k]
            if r >= warmup:
                dev[name].append(d)
                wall[name].append(w)
            if r == warmup + reps - 1:
                stats[name] = report(call, dev[name], wall[name])
                stats[name]["knobs"] = env
    out = stats["default"]
    if variants:
        out["variants"] = {n: {k: stats[n][k] for k in ("knobs", "device_ms", "M_pairs_per_s_device", "tiers", "share_of_hbm_peak")}
                           for n, _ in variants}
    return out


def host_pairs(slab, pairs, overlap):
    """the same numbers on the host for a list of (u, v): dictionaries per row, numpy intersections"""
    ids, sc, lens = slab
    rows = {}

    def row(x):
        if x not in rows:
            k = ids[x, :lens[x]]
            o = np.argsort(k)
            rows[x] = (k[o], sc[x, :lens[x]][o], dict(zip(k.tolist(), sc[x, :lens[x]].tolist())))
        return rows[x]

    fwd, bwd, common = np.zeros(len(pairs)), np.zeros(len(pairs)), np.zeros(len(pairs), dtype=np.int32)
    for j, (u, v) in enumerate(pairs):
        ku, su, du = row(int(u))
        kv, sv, dv = row(int(v))
        fwd[j] = du.get(int(v), 0.0)
        bwd[j] = dv.get(int(u), 0.0)
        if overlap:
            _, ia, ib = np.intersect1d(ku, kv, assume_unique=True, return_indices=True)
            common[j] = len(ia)
            float(np.dot(su[ia], sv[ib]))  # (the naive dot product: what a user would compute)
    return fwd, bwd, common


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--cands", type=int, default=1024)
    ap.add_argument("--baseline", type=int, default=20_000, help="pairs sampled on the host per workload")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: torch brings its own copy of the HIP runtime)
    _build.build()
    out_path = args.out or os.path.join(ROOT, "profiles", f"pairs_rmat{args.scale}_k{args.K}_l{args.L}.json")

    g = ppr.rmat(args.scale, seed=args.seed)
    plan = ppr.GrankPlan(g, args.K, args.L, 0.85, part=g.partitions(), device=0)
    st = plan.run(args.iters, -1.0)
    rng = np.random.default_rng(args.seed)
    info = _lib.lib().ppr_build_info().decode()
    doc = {
        "what": "tools/pairs_bench.py: node-pair scores from the resident baskets",
        "graph": f"RMAT-{args.scale} seed {args.seed}", "n": g.n, "m": g.m, "K": args.K, "L": args.L,
        "iterations_run": int(st.iterations_run), "job_device_ms": float(st.device_ms),
        "library": info, "ppr_src_sha256": info.split("ppr_src_sha256=")[1].split()[0],
        "protocol": f"{args.warmup} warm-up rounds, {args.reps} timed repetitions of the raw C call into arrays allocated once, "
                    "median (min, max); device_ms = HIP events around the kernels; wall_ms = host clock around the call (uploads, "
                    "kernels, downloads); knob variants alternate with the default inside every repetition",
        "hbm_peak_Bps": HBM_PEAK,
        "knobs": {k: os.environ[k] for k in KNOBS if k in os.environ},
    }

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)

    # ---- 1. random pairs, lookup outputs
    u, v = rng.integers(0, g.n, size=args.pairs), rng.integers(0, g.n, size=args.pairs)
    gptr, src, cands, order, _ = ppr.normalize_pairs(u, v)
    probe = Call(plan, gptr, src, cands, ("fwd", "bwd", "hit"))
    doc["random_pairs_probe_only"] = measure(probe, args.warmup, args.reps)
    print("random_pairs_probe_only", json.dumps(doc["random_pairs_probe_only"]), flush=True)
    ranked = Call(plan, gptr, src, cands, ("fwd", "bwd", "hit", "rank", "slen", "clen"))
    doc["random_pairs_with_rank_and_lengths"] = measure(ranked, args.warmup, args.reps)
    print("random_pairs_with_rank_and_lengths", json.dumps(doc["random_pairs_with_rank_and_lengths"]), flush=True)
    save()
    # ---- 2. re-ranking: sources x random candidates, every output
    S = args.sources
    s2 = rng.integers(0, g.n, size=S).astype(np.int32)
    c2 = rng.integers(0, g.n, size=S * args.cands).astype(np.int32)
    g2 = np.arange(S + 1, dtype=np.int64) * args.cands
    rer = Call(plan, g2, s2, c2, OUTS)
    doc[f"rerank_{args.cands}"] = measure(rer, args.warmup, args.reps, [
        ("search_linear", {"PPR_PR_SEARCH": 1}), ("search_binary", {"PPR_PR_SEARCH": 2}),
        ("split_256", {"PPR_PR_SPLIT": 256}), ("split_4096", {"PPR_PR_SPLIT": 4096}), ("all_wave", {"PPR_PR_WAVE_MAX": 1 << 20})])
    print("rerank", json.dumps(doc[f"rerank_{args.cands}"]), flush=True)
    save()
    # ---- 3. every source against the keys of its own row
    # (a one-seed query returns the seed's own row: its keys without downloading the slab)
    q = plan.query([[int(x)] for x in s2], args.L)
    ln3 = q.lens.astype(np.int64)
    g3 = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(ln3, out=g3[1:])
    c3 = np.ascontiguousarray(np.concatenate([q.ids[i, :ln3[i]] for i in range(S)]), dtype=np.int32)
    ownrow = Call(plan, g3, s2, c3, OUTS)
    doc["own_row"] = measure(ownrow, args.warmup, args.reps, [
        ("search_binary", {"PPR_PR_SEARCH": 2}), ("all_wave", {"PPR_PR_WAVE_MAX": 1 << 20}), ("wave_max_64", {"PPR_PR_WAVE_MAX": 64}),
        ("all_workgroup", {"PPR_PR_WAVE_MAX": 0})])
    print("own_row", json.dumps(doc["own_row"]), flush=True)
    save()
    if not args.no_baseline:
        t0 = time.perf_counter()
        slab = plan.fetch_slab()
        t_fetch = time.perf_counter() - t0
        base = {"what": "fetch_slab once, then per pair two dictionary lookups and (overlap workloads) numpy.intersect1d of the two "
                        "sorted rows with a float dot product; timed on a sample and scaled to the workload",
                "fetch_slab_s": t_fetch}
        nb = args.baseline
        for name, call, pairs, overlap in (
                ("random_pairs", probe, list(zip(np.repeat(src, np.diff(gptr))[:nb], cands[:nb])), False),
                (f"rerank_{args.cands}", rer, list(zip(np.repeat(s2, args.cands)[:nb], c2[:nb])), True),
                ("own_row", ownrow, list(zip(np.repeat(s2, ln3)[:nb], c3[:nb])), True)):
            t0 = time.perf_counter()
            fwd, bwd, common = host_pairs(slab, pairs, overlap)
            t = time.perf_counter() - t0
            call()
            k = len(pairs)
            equal = bool(np.array_equal(fwd.view(np.uint64), call.o["fwd"][:k].view(np.uint64))
                         and np.array_equal(bwd.view(np.uint64), call.o["bwd"][:k].view(np.uint64))
                         and (not overlap or np.array_equal(common, call.o["common"][:k])))
            scaled = t * len(call.cands) / max(k, 1)
            base[name] = {"sample_pairs": k, "sample_s": t, "scaled_to_workload_s": scaled,
                          "scaled_with_download_s": scaled + t_fetch, "equal_to_device": equal}
        doc["host_path_for_comparison"] = base
        print("host path", json.dumps(base), flush=True)
        save()
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
