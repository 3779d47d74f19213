"""Throughput of PPR-induced subgraph batches (GrankPlan.subgraphs) on the flagship plan.

Setup: RMAT-22, K64 / L128, after bench.py's 30-iteration job. Workloads: 1,024 and 10,000 uniformly
drawn roots at size 32 and 128 (root_first, COO rows and scores on, int64 indices), and the
10,000-root cases again with max_deg = 2^14.
Protocol: warm-up calls, then >= 10 timed repetitions; per repetition the device_ms (HIP events around
the kernels, uploads and downloads excluded) of a count-only raw call and of the full raw call into
tensors allocated once, and the whole GrankPlan.subgraphs call by the host clock (count call, allocation,
full call). Reported: median, minimum and maximum, N, E, edges walked, G edges/s of the count pass
(edges walked / count-only ms) and of the full call (2 x edges walked / full ms), algo_bytes / device_ms
against the 8 TB/s HBM peak, tier counts, the library digest.
For context: GrankPlan.sweep on the same 10,000 roots (the same walk; its edges/s), and the path a user
has without the feature on 1,000 of the roots: fetch_slab once, then numpy, with the results compared
for equality.
Writes profiles/subgraph_rmat22_k64_l128.json (or --out); nothing in it is asserted anywhere.

    python tools/subgraph_bench.py [--scale 22] [--reps 10] [--no-baseline]
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


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1], "n": len(xs)}


def raw(plan, src, size, max_deg, flags, node_ptr, edge_ptr, ncap, ecap, tensors, st):
    p = [None if t is None else t.data_ptr() for t in tensors]
    return _lib.lib().ppr_grank_plan_subgraphs(plan._p, plan.iterations_run, len(src), _lib.ptr(src), size, max_deg, flags, ncap,
                                               ecap, _lib.ptr(node_ptr), _lib.ptr(edge_ptr), *p, ctypes.byref(st))


def workload(plan, src, size, max_deg, warmup, reps):
    import torch
    flags = _lib.PPR_SUBG_ROOT_FIRST | _lib.PPR_SUBG_IDX64
    S = len(src)
    node_ptr, edge_ptr = np.zeros(S + 1, dtype=np.int64), np.zeros(S + 1, dtype=np.int64)
    st = _lib.PprSubgStats()
    none = (None,) * 6
    _lib.check(raw(plan, src, size, max_deg, flags, node_ptr, edge_ptr, 0, 0, none, st), "count")
    N, E = int(node_ptr[-1]), int(edge_ptr[-1])
    dev = torch.device("cuda", plan.device)
    t = (torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(N + 1, dtype=torch.float64, device=dev),
         torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(E + 1, dtype=torch.int64, device=dev),
         torch.empty(E + 1, dtype=torch.int64, device=dev), None)
    torch.cuda.synchronize()
    cnt_ms, full_ms, call_ms = [], [], []
    for r in range(warmup + reps):
        _lib.check(raw(plan, src, size, max_deg, flags, node_ptr, edge_ptr, 0, 0, none, st), "count")
        c = float(st.device_ms)
        _lib.check(raw(plan, src, size, max_deg, flags, node_ptr, edge_ptr, N, E, t, st), "full")
        f = float(st.device_ms)
        t0 = time.perf_counter()
        b = plan.subgraphs(src, size=size, max_deg=max_deg or None, root_first=True)
        w = (time.perf_counter() - t0) * 1e3
        if r >= warmup:
            cnt_ms.append(c); full_ms.append(f); call_ms.append(w)
    walked = int(st.edges_walked)
    c, f = spread(cnt_ms), spread(full_ms)
    out = {
        "roots": S, "size": size, "max_deg": max_deg or None, "N": N, "E": E, "edges_walked": walked,
        "capped_members": int(st.capped_members),
        "count_only_device_ms": c, "full_device_ms": f, "python_call_ms": spread(call_ms),
        "count_G_edges_per_s": walked / 1e9 / (c["median"] / 1e3) if c["median"] else None,
        "full_G_edges_per_s": 2 * walked / 1e9 / (f["median"] / 1e3) if f["median"] else None,
        "algo_bytes": int(st.algo_bytes), "share_of_hbm_peak": int(st.algo_bytes) / (f["median"] / 1e3) / HBM_PEAK,
        "tiers": {"wave": int(st.wave_sources), "workgroup": int(st.wg_sources), "slice": int(st.slice_sources)},
        "chunks": int(st.chunks),
    }
    return out, b


def numpy_subgraphs(slab, g, sources, size):
    """the same batch on the host, root first: (nodes, rowptr, col) as int64 arrays"""
    ids, sc, lens = slab
    rp, col = g.row_ptr, g.col
    rank = np.full(g.n, -1, dtype=np.int64)
    nodes, rowptr, cols, n0, e0 = [], [], [], 0, 0
    for u in sources:
        k, s = ids[u, :lens[u]].astype(np.int64), sc[u, :lens[u]]
        k = k[np.lexsort((k, -s))]
        at = np.flatnonzero(k == u)
        if len(at):
            k = np.concatenate(([u], np.delete(k, at[0])))
        k = k[:size]
        rank[k] = np.arange(len(k))
        deg = rp[k + 1] - rp[k]
        first = np.repeat(rp[k] - (np.cumsum(deg) - deg), deg)
        rb = rank[col[np.arange(int(deg.sum()), dtype=np.int64) + first] & 0x7fffffff]
        ra = np.repeat(np.arange(len(k)), deg)
        hit = rb >= 0
        per = np.bincount(ra[hit], minlength=len(k))
        rank[k] = -1
        nodes.append(k)
        rowptr.append(e0 + np.cumsum(per) - per)
        cols.append(n0 + rb[hit])
        n0 += len(k)
        e0 += int(hit.sum())
    return np.concatenate(nodes), np.concatenate(rowptr + [np.array([e0])]), np.concatenate(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--baseline", type=int, default=1_000, help="roots sampled on the host for context")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: torch brings its own copy of the HIP runtime)
    _build.build()
    out_path = args.out or os.path.join(ROOT, "profiles", f"subgraph_rmat{args.scale}_k{args.K}_l{args.L}.json")

    g = ppr.rmat(args.scale, seed=args.seed)
    part = g.partitions()
    plan = ppr.GrankPlan(g, args.K, args.L, 0.85, part=part, device=0)
    st = plan.run(args.iters, -1.0)
    rng = np.random.default_rng(args.seed)
    info = _lib.lib().ppr_build_info().decode()
    doc = {
        "what": "tools/subgraph_bench.py: PPR-induced subgraph batches from the resident baskets",
        "graph": f"RMAT-{args.scale} seed {args.seed}", "n": g.n, "m": g.m, "K": args.K, "L": args.L,
        "iterations_run": int(st.iterations_run), "job_device_ms": float(st.device_ms),
        "library": info, "ppr_src_sha256": info.split("ppr_src_sha256=")[1].split()[0],
        "protocol": f"{args.warmup} warm-up rounds, {args.reps} timed repetitions, median (min, max) of the HIP event time "
                    "around the kernels; count-only and full raw calls into tensors allocated once; python_call_ms = host "
                    "clock around GrankPlan.subgraphs (count call, allocation, full call)",
        "hbm_peak_Bps": HBM_PEAK,
        "knobs": {k: os.environ[k] for k in ("PPR_SG_WAVE_MAX", "PPR_SG_WG_MAX", "PPR_SG_SLICE", "PPR_SG_CHUNK") if k in os.environ},
    }
    roots = rng.integers(0, g.n, size=10_000).astype(np.int32)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)

    last = None
    for nroots in (1_024, 10_000):
        for size in (32, 128):
            for max_deg in ((0,) if nroots == 1_024 else (0, 1 << 14)):
                name = f"roots{nroots}_size{size}" + (f"_maxdeg{max_deg}" if max_deg else "")
                doc[name], b = workload(plan, roots[:nroots], size, max_deg, args.warmup, args.reps)
                if nroots == 10_000 and size == 32 and not max_deg:
                    last = b
                print(name, json.dumps(doc[name]), flush=True)
                save()
    # the sweep's walk on the same roots, for context
    dev, sst = [], {}
    for r in range(args.warmup + args.reps):
        plan.sweep(roots, stats=sst)
        if r >= args.warmup:
            dev.append(sst["device_ms"])
    d = spread(dev)
    doc["sweep_for_context"] = {"roots": len(roots), "device_ms": d, "edges": sst["edges"],
                                "G_edges_per_s": sst["edges"] / 1e9 / (d["median"] / 1e3)}
    print("sweep", json.dumps(doc["sweep_for_context"]), flush=True)
    save()
    if not args.no_baseline:
        nb = min(args.baseline, len(roots))
        t0 = time.perf_counter()
        slab = plan.fetch_slab()
        t_fetch = time.perf_counter() - t0
        t0 = time.perf_counter()
        nodes, rowptr, col = numpy_subgraphs(slab, g, roots[:nb], 32)
        t_np = time.perf_counter() - t0
        N, E = int(last.node_ptr[nb]), int(last.edge_ptr[nb])
        doc["host_path_for_context"] = {
            "what": f"fetch_slab once, then {nb} of the roots at size 32 with numpy (lexsort, a rank array over n, bincount)",
            "fetch_slab_s": t_fetch, "numpy_s": t_np, "roots": nb,
            "equal_to_device": bool(np.array_equal(nodes, last.nodes[:N].cpu().numpy())
                                    and np.array_equal(rowptr, last.rowptr[:N + 1].cpu().numpy())
                                    and np.array_equal(col, last.col[:E].cpu().numpy())),
        }
        print("host path", json.dumps(doc["host_path_for_context"]), flush=True)
        save()
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
