"""Latency and throughput of reverse queries (GrankPlan.rquery) on the flagship plan.

Setup: RMAT-22, K64 / L128, after bench.py's 30-iteration job (the protocol of tools/query_bench.py).
Workloads, Kq = 64, targets drawn from the nodes with predecessors:
  single      1 query x 1 target, 64 different targets spread over the in-degree ranks (a frequent
              key has many predecessors), every one through the probe tier and through the scan tier
  set64       1 query x 64 targets
  batch1k     1,024 queries x 6 targets (one chunk)
  batch16k    16,384 queries x 6 targets (16 chunks)
Sweeps: one query of 1, 2, 4, 8, 16 targets with the probe tier forced on and off (the default of
PPR_R_PROBE_MAX is the largest count at which the probe still wins), and PPR_R_SEG on batch1k and on
the most frequent single target.
Protocol: warm-up calls, then >= 10 timed repetitions of the same call; per repetition device_ms (HIP
events around the kernels, uploads and downloads excluded) and the whole call by the host clock.
Reported: median, minimum and maximum of both, and algo_bytes / device_ms against the 8 TB/s HBM peak
(a share of the bandwidth bound). For context only, what a user has without the feature is timed
once: fetch_slab (download + per-row sort of the whole slab), then a numpy column gather for the
set64 targets. Writes profiles/rquery_rmat22_k64_l128.json (or --out); nothing in it is asserted.

    python tools/rquery_bench.py [--scale 22] [--reps 10] [--no-baseline]
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
KNOBS = ("PPR_R_PROBE_MAX", "PPR_R_SEG", "PPR_R_T", "PPR_R_CHUNK", "PPR_R_ENTRIES")


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "n": len(xs)}


class knobs:
    """the library reads its knobs per call"""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def workload(plan, calls, Kq, warmup, reps):
    """`calls`: a list of (qptr, targets); a repetition runs every call once. Timings are per call."""
    for _ in range(warmup):
        for c in calls:
            res = plan.rquery(c, Kq)
    dev, wall = [], []
    per_call = [[] for _ in calls]
    for _ in range(reps):
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            res = plan.rquery(c, Kq)  # synchronous
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(res.device_ms)
            per_call[i].append(res.device_ms)
    d, w = spread(dev), spread(wall)
    Q = len(calls[-1][0]) - 1
    out = {
        "calls": len(calls), "queries_per_call": Q, "targets_per_query": int(len(calls[-1][1]) // max(Q, 1)), "Kq": Kq,
        "device_ms": d, "call_ms": w,
        "queries_per_s_device": Q / (d["median"] / 1e3),
        "last_call": {"hits": res.hits, "algo_bytes": res.algo_bytes, "probe_queries": res.probe_queries,
                      "scan_queries": res.scan_queries, "scans": res.scans, "chunks": res.chunks,
                      "algo_GBps_device": res.algo_bytes / 1e9 / (per_call[-1][len(per_call[-1]) // 2] / 1e3)},
    }
    if len(calls) == 1:
        out["share_of_hbm_peak"] = res.algo_bytes / (d["median"] / 1e3) / HBM_PEAK
    else:
        out["device_ms_median_per_call"] = [float(np.median(x)) for x in per_call]
    return out, res


def one(targets):
    t = np.asarray(targets, dtype=np.int32)
    return np.array([0, len(t)], dtype=np.int64), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--Kq", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _build.build()
    for k in KNOBS:
        os.environ.pop(k, None)
    out_path = args.out or os.path.join(ROOT, "profiles", f"rquery_rmat{args.scale}_k{args.K}_l{args.L}.json")

    g = ppr.rmat(args.scale, seed=args.seed)
    part = g.partitions()
    plan = ppr.GrankPlan(g, args.K, args.L, 0.85, part=part, device=0)
    st = plan.run(args.iters, -1.0)
    indeg = np.bincount(g.col, minlength=g.n)
    by_indeg = np.argsort(-indeg, kind="stable")
    reach = by_indeg[:int((indeg > 0).sum())].astype(np.int32)  # nodes with predecessors, most first
    rng = np.random.default_rng(args.seed)
    info = _lib.lib().ppr_build_info().decode()
    doc = {
        "what": "tools/rquery_bench.py: reverse queries (top sources of a target set) from the resident baskets",
        "graph": f"RMAT-{args.scale} seed {args.seed}", "n": g.n, "m": g.m, "K": args.K, "L": args.L,
        "iterations_run": int(st.iterations_run), "job_device_ms": float(st.device_ms),
        "library": info, "ppr_src_sha256": info.split("ppr_src_sha256=")[1].split()[0],
        "protocol": f"{args.warmup} warm-up calls, {args.reps} timed repetitions, median (min, max); device_ms = HIP "
                    "events around the kernels; call_ms = host clock around the synchronous call (host transposition, "
                    "uploads, kernels, readbacks of the counts, download)",
        "hbm_peak_Bps": HBM_PEAK,
    }

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)

    # 64 single targets over the in-degree ranks, from the largest in-degree down, geometrically spread
    ranks = sorted(set([0, 1, 2, 3] + [int(x) for x in np.geomspace(4, len(reach) - 1, 400)]))
    ranks = [ranks[i] for i in np.linspace(0, len(ranks) - 1, 64).astype(int)]
    singles = [one([reach[r]]) for r in ranks]
    for tier, pm in (("probe", 1 << 20), ("scan", 0)):
        with knobs(PPR_R_PROBE_MAX=pm):
            doc[f"single_{tier}"], _ = workload(plan, singles, args.Kq, args.warmup, args.reps)
        doc[f"single_{tier}"]["in_degree_of_target"] = [int(indeg[reach[r]]) for r in ranks]
        print(f"single_{tier}", json.dumps({k: v for k, v in doc[f"single_{tier}"].items() if "per_call" not in k and
                                            "in_degree" not in k}), flush=True)
        save()
    set64 = rng.choice(reach, size=64, replace=False).astype(np.int32)
    for name, Q, nt in (("set64", 1, 64), ("batch1k", 1024, 6), ("batch16k", 16384, 6)):
        qptr = np.arange(Q + 1, dtype=np.int64) * nt
        targets = set64 if name == "set64" else rng.choice(reach, size=Q * nt).astype(np.int32)
        doc[name], _ = workload(plan, [(qptr, targets)], args.Kq, args.warmup, args.reps)
        print(name, json.dumps(doc[name]), flush=True)
        if name == "batch1k":
            b1k = (qptr, targets)
        save()
    # crossover: one query of 1 .. 16 targets through each tier
    doc["crossover"] = {}
    for np_ in (1, 2, 4, 8, 16):
        call = one(rng.choice(reach, size=np_, replace=False))
        row = {}
        for tier, pm in (("probe", 1 << 20), ("scan", 0)):
            with knobs(PPR_R_PROBE_MAX=pm):
                w, _ = workload(plan, [call], args.Kq, args.warmup, args.reps)
            row[tier] = {"device_ms": w["device_ms"], "call_ms": w["call_ms"], "hits": w["last_call"]["hits"]}
        doc["crossover"][str(np_)] = row
        print("crossover", np_, json.dumps(row), flush=True)
    save()
    # segment size of the list reduction
    doc["seg_sweep"] = {}
    for seg in (1024, 4096, 16384, 65536):
        with knobs(PPR_R_SEG=seg, PPR_R_PROBE_MAX=0):
            a, _ = workload(plan, [b1k], args.Kq, 1, args.reps)
            b, _ = workload(plan, [singles[0]], args.Kq, 1, args.reps)
        doc["seg_sweep"][str(seg)] = {"batch1k_device_ms": a["device_ms"], "top_single_device_ms": b["device_ms"],
                                      "top_single_hits": b["last_call"]["hits"]}
        print("seg", seg, json.dumps(doc["seg_sweep"][str(seg)]), flush=True)
    save()
    if not args.no_baseline:
        t0 = time.perf_counter()
        ids, sc, lens = plan.fetch_slab()
        t_fetch = time.perf_counter() - t0
        t0 = time.perf_counter()
        f = 1.0 / len(set64)
        valid = np.arange(ids.shape[1])[None, :] < lens[:, None]
        rows, cols = np.nonzero(np.isin(ids, set64) & valid)
        score = np.bincount(rows, weights=sc[rows, cols] * f, minlength=g.n)
        cand = np.unique(rows)
        top = cand[np.lexsort((cand, -score[cand]))[:args.Kq]]
        t_gather = time.perf_counter() - t0
        res = plan.rquery(one(set64), args.Kq)
        doc["host_path_for_context"] = {
            "what": "fetch_slab once (download of both slab slots + per-row sort on the host), then the set64 query "
                    "as a numpy column gather over the whole slab (float sums)",
            "fetch_slab_s": t_fetch, "numpy_gather_s": t_gather,
            "top_k_overlap_with_device": len(set(top.tolist()) & set(res.ids[0].tolist())) / args.Kq,
        }
        print("host path", json.dumps(doc["host_path_for_context"]), flush=True)
        save()
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
