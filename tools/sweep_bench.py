"""Throughput of sweep-cut local clustering (GrankPlan.sweep) on the flagship plan.

Setup: RMAT-22, K64 / L128, after bench.py's 30-iteration job. Three workloads:
  all_vol1k   every source, max_vol = 2^10   (short walks: the planner's sort and the wave tier carry it)
  all_vol16k  every source, max_vol = 2^14
  sample      10 K uniformly drawn sources at the default cap floor(m / 2) (hubs are swept: workgroup / slice tiers)
Protocol: warm-up calls, then >= 10 timed repetitions of the same call; per repetition device_ms (HIP
events around the kernels, uploads and downloads excluded) and the whole call by the host clock
(synchronous: upload, kernels, download of the S x L order rows). Reported: median, minimum and maximum
of both, sources/s, edges walked, algo_bytes / device_ms against the 8 TB/s HBM peak (a share of the
bandwidth bound, not a kernel's), tier counts, the library digest.
For context only, the path a user has without the feature is timed on 1,000 of the sample's sources:
fetch_slab once, then the same sweep in numpy (float ratios, not the exact comparison), with the
agreement of the sets reported.
Writes profiles/sweep_rmat22_k64_l128.json (or --out); nothing in it is asserted anywhere.

    python tools/sweep_bench.py [--scale 22] [--reps 10] [--no-baseline]
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


def workload(plan, sources, max_vol, warmup, reps):
    res = None
    for _ in range(warmup):
        res = plan.sweep(sources, max_vol=max_vol)
    dev, call, st = [], [], {}
    for _ in range(reps):
        t0 = time.perf_counter()
        res = plan.sweep(sources, max_vol=max_vol, stats=st)  # synchronous
        call.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["device_ms"])
    S = len(res.size)
    d, c = spread(dev), spread(call)
    found = res.size > 0
    return {
        "sources": S, "max_vol": int(max_vol) if max_vol else "floor(m / 2)",
        "device_ms": d, "call_ms": c,
        "sources_per_s_device": S / (d["median"] / 1e3), "sources_per_s_call": S / (c["median"] / 1e3),
        "edges": st["edges"], "edges_per_s_device": st["edges"] / (d["median"] / 1e3),
        "algo_bytes": st["algo_bytes"], "algo_GBps_device": st["algo_bytes"] / 1e9 / (d["median"] / 1e3),
        "share_of_hbm_peak": st["algo_bytes"] / (d["median"] / 1e3) / HBM_PEAK,
        "tiers": {"wave": st["wave_sources"], "workgroup": st["wg_sources"], "slice": st["slice_sources"]},
        "chunks": st["chunks"],
        "answers": {"with_a_set": int(found.sum()), "mean_swept": float(res.swept.mean()),
                    "mean_size": float(res.size[found].mean()) if found.any() else 0.0,
                    "median_phi": float(np.median(res.phi[found])) if found.any() else None},
    }, res


def numpy_sweep(slab, g, sources, max_vol):
    """the same sweep on the host (float ratios instead of the exact comparison: context for the time only)"""
    ids, sc, lens = slab
    rp, col = g.row_ptr, g.col
    m = int(rp[-1])
    rank = np.full(g.n, -1, dtype=np.int32)
    out = []
    for u in sources:
        k, s = ids[u, :lens[u]].astype(np.int64), sc[u, :lens[u]]
        deg = rp[k + 1] - rp[k]
        o = np.lexsort((k, -(s / np.maximum(deg, 1))))
        k, deg = k[o], deg[o]
        vol = np.cumsum(deg)
        swept = int(np.searchsorted(vol > max_vol, True)) if len(vol) else 0
        k, deg, vol = k[:swept], deg[:swept], vol[:swept]
        if swept == 0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        rank[k] = np.arange(swept, dtype=np.int32)
        W = int(vol[-1])
        ra = np.repeat(np.arange(swept, dtype=np.int32), deg)
        first = np.repeat(rp[k] - (vol - deg), deg)
        rb = rank[col[np.arange(W, dtype=np.int64) + first] & 0x7fffffff]
        hit = rb >= 0
        hist = np.bincount(np.maximum(ra[hit], rb[hit]), minlength=swept)
        rank[k] = -1
        cut = vol - np.cumsum(hist)
        den = np.minimum(vol, m - vol)
        with np.errstate(divide="ignore", invalid="ignore"):
            phi = np.where(den > 0, cut / den, np.inf)
        j = int(np.argmin(phi))
        out.append(k[:j + 1] if np.isfinite(phi[j]) else np.zeros(0, dtype=np.int64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--sample", type=int, default=10_000, help="sources of the default-cap workload")
    ap.add_argument("--baseline", type=int, default=1_000, help="of them, swept on the host for context")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _build.build()
    out_path = args.out or os.path.join(ROOT, "profiles", f"sweep_rmat{args.scale}_k{args.K}_l{args.L}.json")

    g = ppr.rmat(args.scale, seed=args.seed)
    part = g.partitions()
    plan = ppr.GrankPlan(g, args.K, args.L, 0.85, part=part, device=0)
    st = plan.run(args.iters, -1.0)
    rng = np.random.default_rng(args.seed)
    info = _lib.lib().ppr_build_info().decode()
    doc = {
        "what": "tools/sweep_bench.py: sweep-cut local clustering from the resident baskets",
        "graph": f"RMAT-{args.scale} seed {args.seed}", "n": g.n, "m": g.m, "K": args.K, "L": args.L,
        "iterations_run": int(st.iterations_run), "job_device_ms": float(st.device_ms),
        "library": info, "ppr_src_sha256": info.split("ppr_src_sha256=")[1].split()[0],
        "protocol": f"{args.warmup} warm-up calls, {args.reps} timed repetitions, median (min, max); device_ms = HIP "
                    "events around the planner, walk and final kernels; call_ms = host clock around the synchronous call "
                    "(upload, kernels, download of the order rows)",
        "hbm_peak_Bps": HBM_PEAK,
        "knobs": {k: os.environ[k] for k in ("PPR_SW_WAVE_MAX", "PPR_SW_WG_MAX", "PPR_SW_SLICE", "PPR_SW_CHUNK") if k in os.environ},
    }
    sample = rng.integers(0, g.n, size=args.sample).astype(np.int32)
    res = None
    for name, sources, max_vol in (("all_vol1k", None, 1 << 10), ("all_vol16k", None, 1 << 14), ("sample", sample, None)):
        doc[name], res = workload(plan, sources, max_vol, args.warmup, args.reps)
        print(name, json.dumps(doc[name]), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)
    if not args.no_baseline:
        nb = min(args.baseline, len(sample))
        t0 = time.perf_counter()
        slab = plan.fetch_slab()
        t_fetch = time.perf_counter() - t0
        t0 = time.perf_counter()
        sets = numpy_sweep(slab, g, sample[:nb], g.m // 2)
        t_sweep = time.perf_counter() - t0
        dev = res.sets()
        doc["host_path_for_context"] = {
            "what": f"fetch_slab once (download of both slab slots + per-row sort on the host), then {nb} of the sample's "
                    "sources swept with numpy (lexsort, cumsum, a rank array over n, bincount; float ratios)",
            "fetch_slab_s": t_fetch, "numpy_sweep_s": t_sweep, "sources": nb,
            "sets_equal_to_device": float(np.mean([np.array_equal(a, b) for a, b in zip(sets, dev[:nb])])),
        }
        print("host path", json.dumps(doc["host_path_for_context"]), flush=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
