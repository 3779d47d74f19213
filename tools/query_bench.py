"""Throughput of preference-set queries (GrankPlan.query) on the flagship plan.

Setup: RMAT-22, K64 / L128, after bench.py's 30-iteration job. Two workloads, Kq = 64:
  small   1 M queries of 8 uniformly drawn non-dangling seeds   (the wave tier carries it)
  wide    10 K queries of 512 such seeds                        (the workgroup / range tiers)
Protocol: warm-up calls, then >= 10 timed repetitions of the same call; per repetition device_ms
(HIP events around the kernels, upload excluded) and the whole call by the host clock (synchronous:
upload, planner, kernels, download). Reported: median, minimum and maximum of both, queries/s, and
algo_bytes / device_ms against the 8 TB/s HBM peak (a share of the bandwidth bound, not a kernel's).
For context only, the path a user has without the feature is timed on a 1,000-query sample:
fetch_slab once (download + per-row sort of the whole slab), then the same merge in numpy.
Writes profiles/query_rmat22_k64_l128.json (or --out); nothing in it is asserted anywhere.

    python tools/query_bench.py [--scale 22] [--reps 12] [--no-baseline]
"""
import argparse
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


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "n": len(xs)}


def workload(plan, qptr, seeds, Kq, warmup, reps):
    for _ in range(warmup):
        res = plan.query((qptr, seeds), Kq)
    dev, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = plan.query((qptr, seeds), Kq)  # synchronous
        call.append((time.perf_counter() - t0) * 1e3)
        dev.append(res.device_ms)
    Q = len(qptr) - 1
    d, c = spread(dev), spread(call)
    return {
        "queries": Q, "seeds_per_query": int(len(seeds) // max(Q, 1)), "Kq": Kq,
        "device_ms": d, "call_ms": c,
        "queries_per_s_device": Q / (d["median"] / 1e3), "queries_per_s_call": Q / (c["median"] / 1e3),
        "candidates": res.candidates, "algo_bytes": res.algo_bytes,
        "algo_GBps_device": res.algo_bytes / 1e9 / (d["median"] / 1e3),
        "share_of_hbm_peak": res.algo_bytes / (d["median"] / 1e3) / HBM_PEAK,
        "tiers": {"wave": res.wave_queries, "workgroup": res.wg_queries, "range": res.range_queries,
                  "max_ranges": res.max_ranges},
    }, res


def numpy_merge(slab, qptr, seeds, Kq):
    """the same merge on the host (float sums, not the exact ones: context for the time only)"""
    ids, sc, lens = slab
    out = []
    for q in range(len(qptr) - 1):
        s = seeds[qptr[q]:qptr[q + 1]]
        f = 1.0 / len(s)
        k = np.concatenate([ids[u, :lens[u]] for u in s])
        v = np.concatenate([sc[u, :lens[u]] for u in s]) * f
        uk, inv = np.unique(k, return_inverse=True)
        tot = np.bincount(inv, weights=v)
        top = np.lexsort((uk, -tot))[:Kq]
        out.append((uk[top], tot[top]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--Kq", type=int, default=64)
    ap.add_argument("--small", type=int, default=1_000_000, help="queries of 8 seeds")
    ap.add_argument("--wide", type=int, default=10_000, help="queries of 512 seeds")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _build.build()
    out_path = args.out or os.path.join(ROOT, "profiles", f"query_rmat{args.scale}_k{args.K}_l{args.L}.json")

    g = ppr.rmat(args.scale, seed=args.seed)
    part = g.partitions()
    plan = ppr.GrankPlan(g, args.K, args.L, 0.85, part=part, device=0)
    st = plan.run(args.iters, -1.0)
    nd = np.nonzero(g.degrees() > 0)[0].astype(np.int32)
    rng = np.random.default_rng(args.seed)
    info = _lib.lib().ppr_build_info().decode()
    doc = {
        "what": "tools/query_bench.py: preference-set queries from the resident baskets",
        "graph": f"RMAT-{args.scale} seed {args.seed}", "n": g.n, "m": g.m, "K": args.K, "L": args.L,
        "iterations_run": int(st.iterations_run), "job_device_ms": float(st.device_ms),
        "library": info, "ppr_src_sha256": info.split("ppr_src_sha256=")[1].split()[0],
        "protocol": f"{args.warmup} warm-up calls, {args.reps} timed repetitions, median (min, max); device_ms = HIP "
                    "events around the planner and merge kernels; call_ms = host clock around the synchronous call "
                    "(upload, kernels, download)",
        "hbm_peak_Bps": HBM_PEAK,
    }
    sample = None
    for name, Q, ns in (("small", args.small, 8), ("wide", args.wide, 512)):
        qptr = np.arange(Q + 1, dtype=np.int64) * ns
        seeds = rng.choice(nd, size=Q * ns).astype(np.int32)
        doc[name], res = workload(plan, qptr, seeds, args.Kq, args.warmup, args.reps)
        print(name, json.dumps(doc[name]), flush=True)
        if name == "small":
            sample = (qptr[:1001].copy(), seeds[:8 * 1000].copy(), res.ids[:1000].copy())
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
    if not args.no_baseline:
        t0 = time.perf_counter()
        slab = plan.fetch_slab()
        t_fetch = time.perf_counter() - t0
        t0 = time.perf_counter()
        rows = numpy_merge(slab, sample[0], sample[1], args.Kq)
        t_merge = time.perf_counter() - t0
        agree = float(np.mean([len(set(r[0].tolist()) & set(sample[2][q].tolist())) / args.Kq for q, r in enumerate(rows)]))
        doc["host_path_for_context"] = {
            "what": "fetch_slab once (download of both slab slots + per-row sort on the host), then 1,000 of the small "
                    "workload's queries merged with numpy (concatenate, unique, bincount, lexsort; float sums)",
            "fetch_slab_s": t_fetch, "numpy_merge_s_per_1000_queries": t_merge,
            "top_k_overlap_with_device": agree,
        }
        print("host path", json.dumps(doc["host_path_for_context"]), flush=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
