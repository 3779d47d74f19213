// propagate.hip -- feature propagation through a GRank plan's resident baskets, both ways
// (ppr_grank_plan_propagate, ppr_grank_plan_propagate_t; include/ppr_hip.h; device code: propagate.h;
// host planning: prop_plan.h).
//
// Host side of one call: every argument check, the choice of the lane geometry, and for the
// transposed product the passes over key ranges. Knobs, read per call (no result depends on them):
//   PPR_PROP_ENTRIES  E = max(PPR_PROP_ENTRIES, S) postings per pass of the transposed product
//                     (default 2^24, at most 2^30): the sort buffers take 24 E bytes
//   PPR_PROP_PACK     0: the forward kernel gives every position a whole wave (default 1: 64 / G
//                     positions per wave, propagate.h)
//   PPR_PROP_V        1: one column per lane whatever the alignment allows
//   PPR_PROP_HOST_PLAN 1: the chunk tasks are built on the host (prop_plan.h build_chunk_tasks) and uploaded;
//                     default: counted, scanned and written on the device by the same rule
//   PPR_PROP_PART_BYTES  budget of the fp64 partial rows (default 256 MB): wider calls go in column
//                     blocks of whole tiles, never less than one tile
// Transposed, per call: k_p_len gives the postings of the batch; if they fit E the one pass is the
// key range [0, n), otherwise a count pass (k_p_walk<2>, sharded integer counters) gives every key's
// postings and cut_key_ranges the passes. Per pass: count per position, scan, emit in position-major
// order, stable sort by key, run starts, the lists cut into chunk tasks (k_p_tcount, three scans,
// k_p_tplan), k_p_tsum / k_p_tfold / k_p_zero write the range's rows of Y.
// The id-range check and the slot rule are resident_args.h's, the scratch and timing plumbing
// resident_call.h's; both are shared with query.hip and rquery.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "resident_call.h"
#include "propagate.h"

namespace {

using pprprop::ChunkPlan;
using pprprop::KeyRange;
using pprprop::PFold;
using pprprop::PTask;

constexpr int64_t P_ENTRIES_DEFAULT = 1 << 24, P_ENTRIES_MAX = 1 << 30;
constexpr int P_MAX_F = 8192;

// what both directions refuse; sz = bytes of an element
int check_common(const ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources, int32_t F, int32_t dt,
                 uint32_t flags, const void* in, int64_t ldin, const void* out, int64_t ldout) {
  if (!p || p->mc || iterations_run < 0 || S < 0) return PPR_ERR_ARG;
  if (dt != PPR_PROP_F32 && dt != PPR_PROP_BF16) return PPR_ERR_ARG;
  if (flags & ~(uint32_t)PPR_PROP_ROW_NORMALIZE) return PPR_ERR_ARG;
  if (!in || !out) return PPR_ERR_ARG;
  if (!sources && S != p->n) return PPR_ERR_ARG;
  if (F <= 0) return F == 0 ? PPR_ERR_RANGE : PPR_ERR_ARG;
  if (F > P_MAX_F) return PPR_ERR_RANGE;
  if (ldin < F || ldout < F) return PPR_ERR_ARG;
  if (S > P_ENTRIES_MAX) return PPR_ERR_RANGE;  // positions and per-pass offsets are 32-bit
  return sources ? pprres::check_ids(sources, S, p->n) : PPR_OK;
}

// columns per lane: the widest of 16 / 8 bytes that F, both strides and both pointers allow
int pick_v(int32_t dt, int32_t F, const void* a, int64_t lda, const void* b, int64_t ldb) {
  if (env_i64("PPR_PROP_V", 0) == 1) return 1;
  const int esz = dt == PPR_PROP_BF16 ? 2 : 4;
  for (int V = 16 / esz; V >= 4; V >>= 1) {
    const size_t al = (size_t)V * esz;
    if (F % V == 0 && lda % V == 0 && ldb % V == 0 && (uintptr_t)a % al == 0 && (uintptr_t)b % al == 0) return V;
  }
  return 1;
}

// lanes per position of a row walk / of the forward gather: the power of two >= need, 4 .. 64
int pick_lgG(int64_t need) {
  int lgG = 2;
  while (lgG < 6 && ((int64_t)1 << lgG) < need) lgG++;
  return lgG;
}

// the call's sources on the device and the slot rule
int begin_call(ResidentCall& c, PArgs& a, ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
               uint32_t flags, size_t extra_bytes) {
  {
    const int rc = c.begin(p, iterations_run);
    if (rc) return rc;
  }
  {
    const int rc = ensure_scratch(&p->d_p, &p->p_bytes, rnd256(4 * (size_t)std::max<int64_t>(S, 1)) + extra_bytes);
    if (rc) return rc;
  }
  std::memset(&a, 0, sizeof(a));
  a.part = p->d_part;
  a.sA = c.sA;
  a.sB = c.sB;
  a.S = S;
  a.norm = (flags & PPR_PROP_ROW_NORMALIZE) ? 1 : 0;
  a.src = nullptr;
  if (sources && S > 0) {
    HIP_OK(hipMemcpyAsync(p->d_p, sources, 4 * (size_t)S, hipMemcpyHostToDevice, c.s));
    a.src = reinterpret_cast<const int32_t*>(p->d_p);
  }
  return PPR_OK;
}

template <int DT, int V>
void launch_fwd(const ResidentCall& c, const PArgs& a, bool hk, dim3 grid, const void* H, int64_t ldh, void* Z,
                int64_t ldz, int F, int lgG, int64_t ngrp) {
  if (hk) hipLaunchKernelGGL((k_p_fwd<DT, V, true>), grid, dim3(P_THREADS), 0, c.s, c.slab, a, H, ldh, Z, ldz, F, lgG, ngrp);
  else hipLaunchKernelGGL((k_p_fwd<DT, V, false>), grid, dim3(P_THREADS), 0, c.s, c.slab, a, H, ldh, Z, ldz, F, lgG, ngrp);
}

template <int DT, int V>
void launch_tsum(const ResidentCall& c, const PArgs& a, dim3 grid, const double* wpos, const PTask* tasks, int64_t nt,
                 const int64_t* vals, int M, const void* G, int64_t ldg, void* Y, int64_t ldy, double* parts,
                 int64_t nparts, int64_t ldp, int c0, int c1) {
  hipLaunchKernelGGL((k_p_tsum<DT, V>), grid, dim3(P_THREADS), 0, c.s, c.slab, a, wpos, tasks, nt, vals, M, G, ldg, Y, ldy,
                     parts, nparts, ldp, c0, c1);
}

}  // namespace

extern "C" int ppr_grank_plan_device(ppr_plan* p, int32_t* device) {
  if (!p || !device) return PPR_ERR_ARG;
  *device = p->device;
  return PPR_OK;
}

extern "C" int ppr_grank_plan_propagate(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                                        int32_t F, int32_t dt, uint32_t flags, const void* H, int64_t ldh, void* Z,
                                        int64_t ldz, ppr_prop_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  {
    const int rc = check_common(p, iterations_run, S, sources, F, dt, flags, H, ldh, Z, ldz);
    if (rc) return rc;
  }
  if (S == 0 || p->n == 0) return PPR_OK;
  ResidentCall c;
  PArgs a;
  {
    const int rc = begin_call(c, a, p, iterations_run, S, sources, flags, rnd256(8));
    if (rc) return rc;
  }
  const int esz = dt == PPR_PROP_BF16 ? 2 : 4;
  const int V = pick_v(dt, F, H, ldh, Z, ldz);
  const int lgG = env_i64("PPR_PROP_PACK", 1) == 0 ? 6 : pick_lgG((F + V - 1) / V);
  const int G = 1 << lgG, R = WAVE >> lgG;
  const int64_t ngrp = (S + R - 1) / R;
  const dim3 grid((unsigned)((ngrp + P_WPB - 1) / P_WPB), (unsigned)((F + G * V - 1) / (G * V)));
  const bool hk = p->hot_n > 0;
  unsigned long long* d_tot = reinterpret_cast<unsigned long long*>(p->d_p + rnd256(4 * (size_t)S));
  if (st) {  // the postings of the batch (outside the timed span)
    HIP_OK(hipMemsetAsync(d_tot, 0, 8, c.s));
    hipLaunchKernelGGL(k_p_len, dim3((unsigned)((S + P_THREADS - 1) / P_THREADS)), dim3(P_THREADS), 0, c.s, c.slab, a,
                       (double*)nullptr, d_tot);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipEventRecord(p->ev_m0, c.s));
  if (dt == PPR_PROP_F32) {
    if (V == 4) launch_fwd<0, 4>(c, a, hk, grid, H, ldh, Z, ldz, F, lgG, ngrp);
    else launch_fwd<0, 1>(c, a, hk, grid, H, ldh, Z, ldz, F, lgG, ngrp);
  } else {
    if (V == 8) launch_fwd<1, 8>(c, a, hk, grid, H, ldh, Z, ldz, F, lgG, ngrp);
    else if (V == 4) launch_fwd<1, 4>(c, a, hk, grid, H, ldh, Z, ldz, F, lgG, ngrp);
    else launch_fwd<1, 1>(c, a, hk, grid, H, ldh, Z, ldz, F, lgG, ngrp);
  }
  HIP_OK(hipGetLastError());
  {
    const int rc = c.lap();
    if (rc) return rc;
  }
  if (st) {
    unsigned long long tot = 0ull;
    HIP_OK(hipMemcpyAsync(&tot, d_tot, 8, hipMemcpyDeviceToHost, c.s));
    HIP_OK(hipStreamSynchronize(c.s));
    st->device_ms = c.dev_ms;
    st->postings = (int64_t)tot;
    st->algo_bytes = (int64_t)tot * (12 + (int64_t)F * esz) + S * (int64_t)F * esz + 8 * S;
    st->passes = 1;
    st->chunks = 0;
  }
  return PPR_OK;
}

extern "C" int ppr_grank_plan_propagate_t(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                                          int32_t F, int32_t dt, uint32_t flags, const void* Gm, int64_t ldg, void* Y,
                                          int64_t ldy, ppr_prop_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  {
    const int rc = check_common(p, iterations_run, S, sources, F, dt, flags, Gm, ldg, Y, ldy);
    if (rc) return rc;
  }
  const int64_t n = p->n;
  if (n == 0) return PPR_OK;
  const int64_t E = std::max<int64_t>(std::min<int64_t>(std::max<int64_t>(env_i64("PPR_PROP_ENTRIES", P_ENTRIES_DEFAULT), 1),
                                                        P_ENTRIES_MAX), S);
  const bool host_plan = env_i64("PPR_PROP_HOST_PLAN", 0) == 1;
  const int64_t part_budget = std::max<int64_t>(1, env_i64("PPR_PROP_PART_BYTES", (int64_t)256 << 20));
  const int esz = dt == PPR_PROP_BF16 ? 2 : 4;
  const int V = pick_v(dt, F, Gm, ldg, Y, ldy);
  const int tile = WAVE * V;
  const bool hk = p->hot_n > 0;
  const bool norm = (flags & PPR_PROP_ROW_NORMALIZE) != 0;
  const int lgG = pick_lgG(p->L);
  const int Rw = WAVE >> lgG;
  const int64_t ngrp = (S + Rw - 1) / Rw;
  const unsigned wgrid = (unsigned)((ngrp + P_WPB - 1) / P_WPB);
  const size_t Sx = (size_t)std::max<int64_t>(S, 1);

  ResidentCall c;
  PArgs a;
  {
    const size_t extra = rnd256(4 * (Sx + 1)) * 2 + rnd256(8 * Sx) + rnd256(8);
    const int rc = begin_call(c, a, p, iterations_run, S, sources, flags, extra);
    if (rc) return rc;
  }
  hipStream_t s = c.s;
  Carve cv{p->d_p};
  cv.take<int32_t>(Sx);                                // the sources (begin_call)
  int32_t* pcnt = cv.take<int32_t>(Sx + 1);            // a position's keys inside the pass's range
  int32_t* poff = cv.take<int32_t>(Sx + 1);            // their exclusive scan; poff[S] = postings of the pass
  double* wpos = cv.take<double>(Sx);                  // row sums (normalisation)
  unsigned long long* d_tot = cv.take<unsigned long long>(1);

  // ---- the postings of the batch, the row sums
  unsigned long long tot = 0ull;
  if (S > 0) {
    HIP_OK(hipMemsetAsync(d_tot, 0, 8, s));
    HIP_OK(hipEventRecord(p->ev_m0, s));
    hipLaunchKernelGGL(k_p_len, dim3((unsigned)((S + P_THREADS - 1) / P_THREADS)), dim3(P_THREADS), 0, s, c.slab, a,
                       norm ? wpos : (double*)nullptr, d_tot);
    HIP_OK(hipGetLastError());
    const int rc = c.lap();
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(&tot, d_tot, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }

  // ---- the passes
  std::vector<KeyRange> ranges;
  if ((int64_t)tot <= E) {
    ranges.push_back(KeyRange{0, n, (int64_t)tot});
  } else {
    const int rc = ensure_scratch(&p->d_pk, &p->pk_bytes, rnd256(4 * (size_t)n) * (PS_SHARDS + 1));
    if (rc) return rc;
    Carve ck{p->d_pk};
    uint32_t* kc = ck.take<uint32_t>((size_t)n * PS_SHARDS);
    int32_t* kcnt = ck.take<int32_t>((size_t)n);
    HIP_OK(hipMemsetAsync(kc, 0, 4 * (size_t)n * PS_SHARDS, s));
    HIP_OK(hipEventRecord(p->ev_m0, s));
    if (hk) hipLaunchKernelGGL((k_p_walk<true, 2>), dim3(wgrid), dim3(P_THREADS), 0, s, c.slab, a, lgG, ngrp, 0, (int)n,
                               (int32_t*)nullptr, (const int32_t*)nullptr, (uint32_t*)nullptr, (int64_t*)nullptr, 0, kc);
    else hipLaunchKernelGGL((k_p_walk<false, 2>), dim3(wgrid), dim3(P_THREADS), 0, s, c.slab, a, lgG, ngrp, 0, (int)n,
                            (int32_t*)nullptr, (const int32_t*)nullptr, (uint32_t*)nullptr, (int64_t*)nullptr, 0, kc);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_p_kfold, dim3((unsigned)((n + P_THREADS - 1) / P_THREADS)), dim3(P_THREADS), 0, s, kc, n, kcnt);
    HIP_OK(hipGetLastError());
    const int rc2 = c.lap();
    if (rc2) return rc2;
    std::vector<int32_t> h_cnt((size_t)n);
    HIP_OK(hipMemcpyAsync(h_cnt.data(), kcnt, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    ranges = pprprop::cut_key_ranges(h_cnt.data(), n, E);
  }

  int64_t postings = 0, nchunks = 0;
  ChunkPlan plan;
  std::vector<int32_t> h_start;
  for (const KeyRange& kr : ranges) {
    const int64_t nk = kr.k1 - kr.k0;
    // ---- a position's keys inside the range, their offsets
    int M = 0;
    if (S > 0) {
      HIP_OK(hipMemsetAsync(pcnt + S, 0, 4, s));
      size_t tmpb = 0;
      HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, (const int32_t*)pcnt, poff, (int)(S + 1), s));
      // sort arrays are sized below, once M is known; the scan's temporary sits in d_pt until then
      {
        const int rc = ensure_scratch(&p->d_pt, &p->pt_bytes, tmpb);
        if (rc) return rc;
      }
      HIP_OK(hipEventRecord(p->ev_m0, s));
      if (hk) hipLaunchKernelGGL((k_p_walk<true, 0>), dim3(wgrid), dim3(P_THREADS), 0, s, c.slab, a, lgG, ngrp, (int)kr.k0,
                                 (int)kr.k1, pcnt, (const int32_t*)nullptr, (uint32_t*)nullptr, (int64_t*)nullptr, 0,
                                 (uint32_t*)nullptr);
      else hipLaunchKernelGGL((k_p_walk<false, 0>), dim3(wgrid), dim3(P_THREADS), 0, s, c.slab, a, lgG, ngrp, (int)kr.k0,
                              (int)kr.k1, pcnt, (const int32_t*)nullptr, (uint32_t*)nullptr, (int64_t*)nullptr, 0,
                              (uint32_t*)nullptr);
      HIP_OK(hipGetLastError());
      HIP_OK(hipcub::DeviceScan::ExclusiveSum(p->d_pt, tmpb, (const int32_t*)pcnt, poff, (int)(S + 1), s));
      const int rc = c.lap();
      if (rc) return rc;
      HIP_OK(hipMemcpyAsync(&M, poff + S, 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      if (M < 0 || (int64_t)M > E) return PPR_ERR_PROBE;  // (cannot happen: a range holds at most E postings)
    }
    postings += M;

    // ---- the pass's arrays: postings in both sort buffers, digit counts and their scan, run starts
    const int ntiles = (M + PS_TILE - 1) / PS_TILE;
    const size_t Mx = (size_t)std::max(M, 1), nh = (size_t)std::max(ntiles, 1) * 256;
    size_t scanb = 0, kscanb = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, scanb, (const int32_t*)nullptr, (int32_t*)nullptr, (int)nh, s));
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, kscanb, (const int32_t*)nullptr, (int32_t*)nullptr, (int)(nk + 1), s));
    {
      const size_t need = 2 * rnd256(4 * Mx) + 2 * rnd256(8 * Mx) + 2 * rnd256(4 * nh) + rnd256(scanb) +
                          rnd256(4 * (size_t)(nk + 1)) * (host_plan ? 1 : 7) + rnd256(kscanb);
      const int rc = ensure_scratch(&p->d_ps, &p->ps_bytes, need);
      if (rc) return rc;
    }
    Carve cs{p->d_ps};
    uint32_t* kbuf[2] = {cs.take<uint32_t>(Mx), cs.take<uint32_t>(Mx)};
    int64_t* vbuf[2] = {cs.take<int64_t>(Mx), cs.take<int64_t>(Mx)};
    int32_t* hist = cs.take<int32_t>(nh);
    int32_t* offs = cs.take<int32_t>(nh);
    unsigned char* scan_tmp = cs.take<unsigned char>(std::max<size_t>(scanb, 1));
    int32_t* kstart = cs.take<int32_t>((size_t)(nk + 1));
    int32_t *tcnt[3] = {nullptr, nullptr, nullptr}, *toffs[3] = {nullptr, nullptr, nullptr};  // tasks | partial rows | folds
    if (!host_plan)
      for (int q = 0; q < 3; q++) { tcnt[q] = cs.take<int32_t>((size_t)(nk + 1)); toffs[q] = cs.take<int32_t>((size_t)(nk + 1)); }
    unsigned char* kscan_tmp = cs.take<unsigned char>(std::max<size_t>(kscanb, 1));
    const unsigned kgrid = (unsigned)((nk + 1 + P_THREADS - 1) / P_THREADS);
    int cur = 0;
    HIP_OK(hipEventRecord(p->ev_m0, s));
    if (M > 0) {
      if (hk) hipLaunchKernelGGL((k_p_walk<true, 1>), dim3(wgrid), dim3(P_THREADS), 0, s, c.slab, a, lgG, ngrp, (int)kr.k0,
                                 (int)kr.k1, (int32_t*)nullptr, (const int32_t*)poff, kbuf[0], vbuf[0], M, (uint32_t*)nullptr);
      else hipLaunchKernelGGL((k_p_walk<false, 1>), dim3(wgrid), dim3(P_THREADS), 0, s, c.slab, a, lgG, ngrp, (int)kr.k0,
                              (int)kr.k1, (int32_t*)nullptr, (const int32_t*)poff, kbuf[0], vbuf[0], M, (uint32_t*)nullptr);
      HIP_OK(hipGetLastError());
      // ---- stable sort by key - k0 < nk, 8 bits per pass
      const unsigned sgrid = (unsigned)((ntiles + P_WPB - 1) / P_WPB);
      for (int shift = 0; shift < 32 && ((nk - 1) >> shift) != 0; shift += 8) {
        hipLaunchKernelGGL(k_p_scount, dim3(sgrid), dim3(P_THREADS), 0, s, (const uint32_t*)kbuf[cur], M, shift, hist, ntiles);
        HIP_OK(hipGetLastError());
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scanb, (const int32_t*)hist, offs, (int)nh, s));
        hipLaunchKernelGGL(k_p_sscatter, dim3(sgrid), dim3(P_THREADS), 0, s, (const uint32_t*)kbuf[cur],
                           (const int64_t*)vbuf[cur], kbuf[cur ^ 1], vbuf[cur ^ 1], M, shift, (const int32_t*)offs, ntiles);
        HIP_OK(hipGetLastError());
        cur ^= 1;
      }
    }
    hipLaunchKernelGGL(k_p_kstart, dim3(kgrid), dim3(P_THREADS), 0, s,
                       (const uint32_t*)kbuf[cur], M, nk, kstart);
    HIP_OK(hipGetLastError());
    {
      const int rc = c.lap();
      if (rc) return rc;
    }
    // ---- the chunk tasks: counted and written on the device (PPR_PROP_HOST_PLAN=1: the host builder)
    int64_t nt = 0, nf = 0, nparts = 0;
    if (host_plan) {
      h_start.resize((size_t)(nk + 1));
      HIP_OK(hipMemcpyAsync(h_start.data(), kstart, 4 * (size_t)(nk + 1), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      pprprop::build_chunk_tasks(h_start.data(), nk, kr.k0, pprprop::PROP_CHUNK, plan);
      nt = (int64_t)plan.tasks.size();
      nf = (int64_t)plan.folds.size();
      nparts = plan.nparts;
    } else {
      HIP_OK(hipEventRecord(p->ev_m0, s));
      hipLaunchKernelGGL(k_p_tcount, dim3(kgrid), dim3(P_THREADS), 0, s, (const int32_t*)kstart, nk, tcnt[0], tcnt[1], tcnt[2]);
      HIP_OK(hipGetLastError());
      for (int q = 0; q < 3; q++)
        HIP_OK(hipcub::DeviceScan::ExclusiveSum(kscan_tmp, kscanb, (const int32_t*)tcnt[q], toffs[q], (int)(nk + 1), s));
      const int rc = c.lap();
      if (rc) return rc;
      int32_t tot3[3] = {0, 0, 0};
      for (int q = 0; q < 3; q++) HIP_OK(hipMemcpyAsync(&tot3[q], toffs[q] + nk, 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      if (tot3[0] < 0 || tot3[1] < 0 || tot3[2] < 0) return PPR_ERR_PROBE;  // (cannot happen: at most M / 512 + nk tasks)
      nt = tot3[0];
      nparts = tot3[1];
      nf = tot3[2];
    }
    nchunks += nt;
    const int cb = pprprop::prop_col_block(nparts, F, tile, part_budget);
    const int64_t ldp = cb;
    {
      const size_t need = rnd256(sizeof(PTask) * (size_t)std::max<int64_t>(nt, 1)) +
                          rnd256(sizeof(PFold) * (size_t)std::max<int64_t>(nf, 1)) +
                          rnd256(8 * (size_t)std::max<int64_t>(nparts, 1) * (size_t)ldp);
      const int rc = ensure_scratch(&p->d_pt, &p->pt_bytes, need);
      if (rc) return rc;
    }
    Carve ct{p->d_pt};
    PTask* d_tasks = ct.take<PTask>((size_t)std::max<int64_t>(nt, 1));
    PFold* d_folds = ct.take<PFold>((size_t)std::max<int64_t>(nf, 1));
    double* parts = ct.take<double>((size_t)std::max<int64_t>(nparts, 1) * (size_t)ldp);
    if (host_plan) {
      if (nt) HIP_OK(hipMemcpyAsync(d_tasks, plan.tasks.data(), sizeof(PTask) * (size_t)nt, hipMemcpyHostToDevice, s));
      if (nf) HIP_OK(hipMemcpyAsync(d_folds, plan.folds.data(), sizeof(PFold) * (size_t)nf, hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipEventRecord(p->ev_m0, s));
    if (!host_plan && nt) {
      hipLaunchKernelGGL(k_p_tplan, dim3(kgrid), dim3(P_THREADS), 0, s, (const int32_t*)kstart, nk, kr.k0,
                         (const int32_t*)toffs[0], (const int32_t*)toffs[1], (const int32_t*)toffs[2], d_tasks, nt, d_folds,
                         nf);
      HIP_OK(hipGetLastError());
    }
    for (int c0 = 0; c0 < F && nt > 0; c0 += cb) {
      const int c1 = std::min(F, c0 + cb);
      const dim3 grid((unsigned)((nt + P_WPB - 1) / P_WPB), (unsigned)((c1 - c0 + tile - 1) / tile));
      const int64_t* vals = vbuf[cur];
      if (dt == PPR_PROP_F32) {
        if (V == 4) launch_tsum<0, 4>(c, a, grid, wpos, d_tasks, nt, vals, M, Gm, ldg, Y, ldy, parts, nparts, ldp, c0, c1);
        else launch_tsum<0, 1>(c, a, grid, wpos, d_tasks, nt, vals, M, Gm, ldg, Y, ldy, parts, nparts, ldp, c0, c1);
      } else {
        if (V == 8) launch_tsum<1, 8>(c, a, grid, wpos, d_tasks, nt, vals, M, Gm, ldg, Y, ldy, parts, nparts, ldp, c0, c1);
        else if (V == 4) launch_tsum<1, 4>(c, a, grid, wpos, d_tasks, nt, vals, M, Gm, ldg, Y, ldy, parts, nparts, ldp, c0, c1);
        else launch_tsum<1, 1>(c, a, grid, wpos, d_tasks, nt, vals, M, Gm, ldg, Y, ldy, parts, nparts, ldp, c0, c1);
      }
      HIP_OK(hipGetLastError());
      if (nf) {
        if (dt == PPR_PROP_F32)
          hipLaunchKernelGGL((k_p_tfold<0>), dim3((unsigned)nf), dim3(P_THREADS), 0, s, c.slab, (const PFold*)d_folds,
                             (const double*)parts, nparts, ldp, Y, ldy, c0, c1);
        else
          hipLaunchKernelGGL((k_p_tfold<1>), dim3((unsigned)nf), dim3(P_THREADS), 0, s, c.slab, (const PFold*)d_folds,
                             (const double*)parts, nparts, ldp, Y, ldy, c0, c1);
        HIP_OK(hipGetLastError());
      }
    }
    {  // (a key with postings is left alone)
      const dim3 zgrid((unsigned)((nk + P_WPB - 1) / P_WPB));
      if (dt == PPR_PROP_F32)
        hipLaunchKernelGGL((k_p_zero<0>), zgrid, dim3(P_THREADS), 0, s, (const int32_t*)kstart, nk, kr.k0, Y, ldy, (int)F);
      else
        hipLaunchKernelGGL((k_p_zero<1>), zgrid, dim3(P_THREADS), 0, s, (const int32_t*)kstart, nk, kr.k0, Y, ldy, (int)F);
      HIP_OK(hipGetLastError());
    }
    {
      const int rc = c.lap();  // (waits: the pass's arrays are reused by the next one)
      if (rc) return rc;
    }
  }
  HIP_OK(hipStreamSynchronize(s));
  if (st) {
    st->device_ms = c.dev_ms;
    st->postings = postings;
    st->algo_bytes = postings * (12 + (int64_t)F * esz) + n * (int64_t)F * esz + 8 * S;
    st->passes = (int64_t)ranges.size();
    st->chunks = (int32_t)std::min<int64_t>(nchunks, INT32_MAX);
  }
  return PPR_OK;
}
