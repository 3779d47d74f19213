"""Feature propagation through the resident table (GrankPlan.propagate / propagate_t) on the flagship plan.

Setup: RMAT-22, K64 / L128, after bench.py's 30-iteration job. Shapes, F = 64 and 256, fp32 and bf16:
  fwd_all     Z = B H over every source, in order
  fwd_batch   Z = B[S] H over a batch of 65,536 uniformly drawn sources
  t_batch     Y = B[S]^T G over the same batch
Protocol (tools/query_bench.py's): 2 warm-up calls, then >= 10 timed repetitions of the same call; per
repetition device_ms (HIP events around the kernels) and the whole synchronous call by the host
clock. Reported: median (min, max), algo_bytes / device_ms as a share of the 8 TB/s HBM peak (a
share of the bandwidth bound of the whole product, not a kernel's), and the ratio to the baseline.
Baseline, in the same session on the same box: what a user had before -- fetch_slab (timed
separately), a torch.sparse_csr_tensor of the rows on the device, torch.sparse.mm in fp32 (device
time by torch events, same warm-up and repetitions; the sparse tensor's construction is timed apart).
Writes profiles/propagate_rmat22_k64_l128.json (or --out); nothing in it is asserted anywhere.

    python tools/propagate_bench.py [--scale 22] [--reps 10] [--no-baseline]
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


def timed(call, warmup, reps):
    """call(stats) -> result; device_ms from the stats, call_ms by the host clock"""
    st = {}
    for _ in range(warmup):
        call(st)
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(st)  # synchronous
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["device_ms"])
    d = spread(dev)
    return {"device_ms": d, "call_ms": spread(wall), "postings": st["postings"], "algo_bytes": st["algo_bytes"],
            "passes": st["passes"], "chunks": st["chunks"],
            "algo_GBps_device": st["algo_bytes"] / 1e9 / (d["median"] / 1e3),
            "share_of_hbm_peak": st["algo_bytes"] / (d["median"] / 1e3) / HBM_PEAK}


def torch_timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(float(e0.elapsed_time(e1)))
    return spread(ms)


def csr_of(torch, slab, rows):
    """fp32 torch.sparse_csr_tensor [len(rows), n] of the slab's rows, on the device"""
    ids, sc, lens = slab
    ln = lens[rows].astype(np.int64)
    crow = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(ln, out=crow[1:])
    mask = np.arange(ids.shape[1])[None, :] < ln[:, None]
    col = ids[rows][mask].astype(np.int64)
    val = sc[rows][mask].astype(np.float32)
    return torch.sparse_csr_tensor(torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(),
                                   torch.from_numpy(val).cuda(), size=(len(rows), ids.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    _build.build()
    out_path = args.out or os.path.join(ROOT, "profiles", f"propagate_rmat{args.scale}_k{args.K}_l{args.L}.json")

    g = ppr.rmat(args.scale, seed=args.seed)
    part = g.partitions()
    plan = ppr.GrankPlan(g, args.K, args.L, 0.85, part=part, device=0)
    st = plan.run(args.iters, -1.0)
    rng = np.random.default_rng(args.seed)
    batch = rng.integers(0, g.n, size=args.batch).astype(np.int32)
    info = _lib.lib().ppr_build_info().decode()
    doc = {
        "what": "tools/propagate_bench.py: feature propagation through the resident baskets, both ways",
        "graph": f"RMAT-{args.scale} seed {args.seed}", "n": g.n, "m": g.m, "K": args.K, "L": args.L,
        "iterations_run": int(st.iterations_run), "job_device_ms": float(st.device_ms), "batch": int(args.batch),
        "library": info, "ppr_src_sha256": info.split("ppr_src_sha256=")[1].split()[0],
        "protocol": f"{args.warmup} warm-up calls, {args.reps} timed repetitions, median (min, max); device_ms = HIP "
                    "events around the kernels; call_ms = host clock around the synchronous call (source upload, "
                    "scans and size read-backs between the kernels)",
        "hbm_peak_Bps": HBM_PEAK, "shapes": {},
    }

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)

    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    feats = {}
    for F in (64, 256):
        H32 = torch.randn((g.n, F), device="cuda", generator=gen)
        G32 = torch.randn((args.batch, F), device="cuda", generator=gen)
        feats[F] = (H32, G32)
        for kind, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            H, G = H32.to(dtype), G32.to(dtype)
            Zall = torch.empty((g.n, F), dtype=dtype, device="cuda")
            Zb = torch.empty((args.batch, F), dtype=dtype, device="cuda")
            Y = torch.empty((g.n, F), dtype=dtype, device="cuda")
            r = {
                "fwd_all": timed(lambda s: plan.propagate(H, out=Zall, stats=s), args.warmup, args.reps),
                "fwd_batch": timed(lambda s: plan.propagate(H, batch, out=Zb, stats=s), args.warmup, args.reps),
                "t_batch": timed(lambda s: plan.propagate_t(G, batch, out=Y, stats=s), args.warmup, args.reps),
            }
            doc["shapes"][f"F{F}_{kind}"] = r
            print(f"F{F}_{kind}", json.dumps(r), flush=True)
            save()
            del H, G, Zall, Zb, Y

    if not args.no_baseline:
        base = {"what": "fetch_slab, torch.sparse_csr_tensor on the device, torch.sparse.mm in fp32 (torch events)"}
        t0 = time.perf_counter()
        slab = plan.fetch_slab()
        base["fetch_slab_s"] = time.perf_counter() - t0
        print("fetch_slab_s", base["fetch_slab_s"], flush=True)
        try:
            t0 = time.perf_counter()
            A = csr_of(torch, slab, np.arange(g.n))
            torch.cuda.synchronize()
            base["build_csr_all_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            Ab = csr_of(torch, slab, batch.astype(np.int64))
            AbT = Ab.to_sparse_coo().t().coalesce().to_sparse_csr()  # the adjoint needs its own index
            torch.cuda.synchronize()
            base["build_csr_batch_and_transpose_s"] = time.perf_counter() - t0
            base["nnz_all"], base["nnz_batch"] = int(A._nnz()), int(Ab._nnz())
            for F in (64, 256):
                H32, G32 = feats[F]
                b = {"fwd_all_ms": torch_timed(torch, lambda: torch.sparse.mm(A, H32), args.warmup, args.reps),
                     "fwd_batch_ms": torch_timed(torch, lambda: torch.sparse.mm(Ab, H32), args.warmup, args.reps),
                     "t_batch_ms": torch_timed(torch, lambda: torch.sparse.mm(AbT, G32), args.warmup, args.reps)}
                base[f"F{F}_fp32"] = b
                print(f"baseline F{F}", json.dumps(b), flush=True)
                for kind in ("fp32", "bf16"):
                    r = doc["shapes"][f"F{F}_{kind}"]
                    for shape in ("fwd_all", "fwd_batch", "t_batch"):
                        r[shape]["baseline_ms_over_device_ms"] = b[shape + "_ms"]["median"] / r[shape]["device_ms"]["median"]
                        r[shape]["baseline_ms_over_call_ms"] = b[shape + "_ms"]["median"] / r[shape]["call_ms"]["median"]
        except Exception as e:  # (a torch build without sparse CSR kernels: say so instead of failing the run)
            base["error"] = f"{type(e).__name__}: {e}"
            print("baseline failed:", base["error"], flush=True)
        doc["baseline"] = base
        save()
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
