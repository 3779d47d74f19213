// subgraph.hip -- PPR-induced subgraph batches from a GRank plan's resident baskets
// (ppr_grank_plan_subgraphs; include/ppr_hip.h; device code: subgraph.h; host planning and the
// refusals: subgraph_plan.h).
//
// Host side of one call: every argument check, the chunks, a chunk's walk batches, the tier lists
// of a batch and the slice tasks. Knobs, read per call (no result depends on them):
//   PPR_SG_WAVE_MAX  a source whose walk has at most this many edges (and at most 192 members) is
//                    answered by one wave (default 2048; 0: no source goes to the wave tier)
//   PPR_SG_WG_MAX    ... at most this many edges by one workgroup (default 2^17; 0: none)
//   PPR_SG_SLICE     edges per (source, slice) workgroup beyond that (default 2^15, at least 64;
//                    rounded down to whole 64-edge groups)
//   PPR_SG_CHUNK     sources per chunk (default 2^15; a chunk also holds at most 2^21 row entries)
// Per chunk: k_g_plan orders every row, cuts it and gives the verdicts; the host scans the member
// counts into node_ptr and cuts the chunk into walk batches of bounded groups and members, so that
// the scratch cached on the plan does not grow with S or with the edges walked. Per batch: the count
// pass (k_g_wave / k_g_wg, one launch per table size / k_g_slice), the scans of the per-member and
// per-group counts (hipcub::DeviceScan), rowptr and edge_ptr, the capacity check, and -- only when
// every edge so far fits -- the emit pass, the same walk with the same numbering.
// The slot rule is resident_args.h's, the scratch and timing plumbing resident_call.h's; both are
// shared with query.hip, rquery.hip, propagate.hip and sweep.hip.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "resident_call.h"
#include "subgraph.h"

namespace {

using pprsubg::GTask;

// device arrays of one chunk of nq sources, carved from ppr_plan::d_sg
struct GChunkDev {
  int32_t *src, *order, *cnt, *code, *capm, *rlen, *list;
  uint64_t* scb;
  int64_t *W, *ngr, *noff, *goff, *eptr;
  size_t bytes;
  GChunkDev(unsigned char* base, int64_t nq, int64_t width) {
    Carve c{base};
    const size_t q = (size_t)std::max<int64_t>(nq, 1), e = q * (size_t)std::max<int64_t>(width, 1);
    src = c.take<int32_t>(q);
    order = c.take<int32_t>(e);
    scb = c.take<uint64_t>(e);
    cnt = c.take<int32_t>(q);
    W = c.take<int64_t>(q);
    ngr = c.take<int64_t>(q);
    code = c.take<int32_t>(q);
    capm = c.take<int32_t>(q);
    rlen = c.take<int32_t>(q);
    noff = c.take<int64_t>(q + 1);
    goff = c.take<int64_t>(q);
    eptr = c.take<int64_t>(q);
    list = c.take<int32_t>(q);
    bytes = c.off;
  }
};

// device arrays of one walk batch, carved from ppr_plan::d_sgh
struct GBatchDev {
  unsigned long long* mc;
  int64_t* roff;
  int32_t *gcnt, *gbase;
  GTask* tasks;
  unsigned char* tmp;
  size_t bytes;
  GBatchDev(unsigned char* base, int64_t Nb, int64_t Gb, int64_t nt, size_t tmpb) {
    Carve c{base};
    mc = c.take<unsigned long long>((size_t)Nb + 1);
    roff = c.take<int64_t>((size_t)Nb + 1);
    gcnt = c.take<int32_t>((size_t)Gb + 1);
    gbase = c.take<int32_t>((size_t)Gb + 1);
    tasks = c.take<GTask>((size_t)std::max<int64_t>(nt, 1));
    tmp = c.take<unsigned char>(std::max<size_t>(tmpb, 1));
    bytes = c.off;
  }
};

struct SubgOut {
  int64_t node_cap, edge_cap;
  int64_t *node_ptr, *edge_ptr;
  void *nodes, *rowptr, *col, *row;
  double* scores;
  int64_t* eid;
};

int subg_core(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources, int64_t width, int64_t max_deg,
              bool root_first, bool idx64, const SubgOut& out, ppr_subg_stats* st) {
  const bool count_only = out.nodes == nullptr;
  const int isz = idx64 ? 8 : 4;

  // test knobs, read per call
  const int64_t wave_max = pprsubg::clamp_wave_max(env_i64("PPR_SG_WAVE_MAX", pprsubg::SG_WAVE_MAX_DEFAULT));
  const int64_t wg_max = pprsubg::clamp_wg_max(env_i64("PPR_SG_WG_MAX", pprsubg::SG_WG_MAX_DEFAULT));
  const int64_t per_task = pprsubg::slice_groups(env_i64("PPR_SG_SLICE", pprsubg::SG_SLICE_DEFAULT));
  const int64_t chunk_rows = std::max<int64_t>(1, env_i64("PPR_SG_CHUNK", pprsubg::SG_CHUNK_DEFAULT));

  ResidentCall call;
  {
    const int rc = call.begin(p, iterations_run);
    if (rc) return rc;
  }
  hipStream_t s = call.s;
  int Lp = WAVE;
  while (Lp < p->L) Lp <<= 1;
  const int plan_wpb = Lp <= 1024 ? pprk::G_WPB : 1;
  const bool hk = p->hot_n > 0;
  {
    int rc = set_lds((const void*)k_g_wg<false>, g_lds(pprsubg::SG_MAX_T));
    if (!rc) rc = set_lds((const void*)k_g_wg<true>, g_lds(pprsubg::SG_MAX_T));
    if (!rc) rc = set_lds((const void*)k_g_slice<false>, g_lds(pprsubg::SG_MAX_T));
    if (!rc) rc = set_lds((const void*)k_g_slice<true>, g_lds(pprsubg::SG_MAX_T));
    if (rc) return rc;
  }

  const std::vector<int64_t> cb = pprsubg::cut_chunks(S, std::max<int64_t>(width, p->L), chunk_rows, pprsubg::SG_CHUNK_ENTRIES);
  std::vector<int32_t> code, rlen, cnt, capm, list;
  std::vector<int64_t> W, ngr, noff, goff, Gl;
  std::vector<GTask> tasks;
  int64_t N = 0, E = 0, walked = 0, walked_emit = 0, groups = 0, entries = 0, capped = 0, E_emit = 0;
  int64_t nwave = 0, nwg = 0, nslice = 0;
  bool fits = !count_only;  // every edge counted so far may be written
  out.node_ptr[0] = 0;
  out.edge_ptr[0] = 0;
  for (size_t c = 0; c + 1 < cb.size(); c++) {
    const int64_t q0 = cb[c], q1 = cb[c + 1], nq = q1 - q0;
    {
      const int rc = ensure_scratch(&p->d_sg, &p->sg_bytes, GChunkDev(nullptr, nq, width).bytes);
      if (rc) return rc;
    }
    const GChunkDev d(p->d_sg, nq, width);
    GArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src_base = q0;
    a.part = p->d_part;
    a.sA = call.sA;
    a.sB = call.sB;
    a.rp = p->d_rp;
    a.colx = p->d_colx;
    a.n = p->n;
    a.width = (int)width;
    a.root_first = root_first ? 1 : 0;
    a.idx64 = idx64 ? 1 : 0;
    a.max_deg = max_deg;
    a.order = d.order; a.scb = d.scb; a.cnt = d.cnt; a.W = d.W; a.ngr = d.ngr; a.code = d.code; a.capm = d.capm;
    a.rlen = d.rlen; a.noff = d.noff; a.goff = d.goff; a.eptr = d.eptr;
    a.node_cap = out.node_cap; a.edge_cap = out.edge_cap;
    a.nodes = out.nodes; a.scores = out.scores; a.rowptr = out.rowptr; a.col = out.col; a.row = out.row; a.eid = out.eid;
    if (sources) {
      HIP_OK(hipMemcpyAsync(d.src, sources + q0, 4 * (size_t)nq, hipMemcpyHostToDevice, s));
      a.src = d.src;
    }
    // ---- the members in order, the verdicts
    {
      const dim3 grid((unsigned)((nq + plan_wpb - 1) / plan_wpb)), block(plan_wpb * WAVE);
      const size_t lds = plan_wpb * g_plan_lds(Lp);
      HIP_OK(hipEventRecord(p->ev_m0, s));
      if (hk) hipLaunchKernelGGL((k_g_plan<true>), grid, block, lds, s, call.slab, a, nq, Lp, wave_max, wg_max);
      else hipLaunchKernelGGL((k_g_plan<false>), grid, block, lds, s, call.slab, a, nq, Lp, wave_max, wg_max);
      HIP_OK(hipGetLastError());
      const int rc = call.lap();
      if (rc) return rc;
    }
    code.resize((size_t)nq); rlen.resize((size_t)nq); cnt.resize((size_t)nq); capm.resize((size_t)nq);
    W.resize((size_t)nq); ngr.resize((size_t)nq);
    HIP_OK(hipMemcpyAsync(code.data(), d.code, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(rlen.data(), d.rlen, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(cnt.data(), d.cnt, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(capm.data(), d.capm, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(W.data(), d.W, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(ngr.data(), d.ngr, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    // ---- node_ptr, the walk batches, every source's first group within its batch
    noff.resize((size_t)nq + 1);
    goff.resize((size_t)nq);
    noff[0] = N;
    for (int64_t q = 0; q < nq; q++) {
      if (W[q] > pprsubg::SG_EDGE_LIMIT || W[q] < 0 || cnt[q] < 0 || cnt[q] > width) return PPR_ERR_RANGE;
      noff[q + 1] = noff[q] + cnt[q];
      out.node_ptr[q0 + q + 1] = noff[q + 1];
      walked += W[q];
      entries += rlen[q];
      capped += capm[q];
      groups += ngr[q];
    }
    N = noff[nq];
    const std::vector<int64_t> bb =
        pprsubg::cut_batches(ngr.data(), cnt.data(), nq, pprsubg::SG_BATCH_GROUPS, pprsubg::SG_BATCH_MEMBERS);
    for (size_t b = 0; b + 1 < bb.size(); b++) {
      int64_t g = 0;
      for (int64_t q = bb[b]; q < bb[b + 1]; q++) {
        goff[q] = g;
        g += ngr[q];
      }
    }
    HIP_OK(hipMemcpyAsync(d.noff, noff.data(), 8 * ((size_t)nq + 1), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d.goff, goff.data(), 8 * (size_t)nq, hipMemcpyHostToDevice, s));
    if (!count_only) {
      const int64_t nt = nq * width;
      HIP_OK(hipEventRecord(p->ev_m0, s));
      hipLaunchKernelGGL(k_g_nodes, dim3((unsigned)((nt + pprk::G_FLAT_THREADS - 1) / pprk::G_FLAT_THREADS)),
                         dim3(pprk::G_FLAT_THREADS), 0, s, a, nq);
      HIP_OK(hipGetLastError());
      const int rc = call.lap();
      if (rc) return rc;
    }
    for (size_t b = 0; b + 1 < bb.size(); b++) {
      const int64_t b0 = bb[b], b1 = bb[b + 1], nb = b1 - b0;
      const int64_t Nb = noff[b1] - noff[b0];
      int64_t Gb = 0, Wb = 0;
      for (int64_t q = b0; q < b1; q++) {
        Gb += ngr[q];
        Wb += W[q];
      }
      if (Nb + 1 > 0x7fffffff || Gb + 1 > 0x7fffffff) return PPR_ERR_RANGE;  // (cannot happen: the budgets, the edge limit)
      // ---- tier lists (chunk indices, in source order): wave | workgroup by table size | slices
      constexpr int WG0 = 1, NWG = 6, SL = WG0 + NWG, NTIER = SL + 1;
      int64_t tc[NTIER] = {}, beg[NTIER + 1] = {};
      auto tier_of = [&](int cq) {
        if (cq == pprsubg::SG_CODE_WAVE) return 0;
        if (cq >= pprsubg::SG_CODE_SLICE) return SL;
        return WG0 + std::max(0, std::min(NWG - 1, cq - pprsubg::SG_CODE_WG - 8));
      };
      for (int64_t q = b0; q < b1; q++) tc[tier_of(code[q])]++;
      for (int t = 0; t < NTIER; t++) beg[t + 1] = beg[t] + tc[t];
      list.resize((size_t)nb);
      {
        int64_t fill[NTIER];
        std::copy(beg, beg + NTIER, fill);
        for (int64_t q = b0; q < b1; q++) list[fill[tier_of(code[q])]++] = (int32_t)q;
      }
      nwave += tc[0];
      nslice += tc[SL];
      nwg += nb - tc[0] - tc[SL];
      int max_members = 0;
      Gl.resize((size_t)tc[SL]);
      for (int64_t i = 0; i < tc[SL]; i++) {
        const int32_t q = list[beg[SL] + i];
        Gl[i] = ngr[q];
        max_members = std::max(max_members, cnt[q]);
      }
      pprsubg::cut_slices(list.data() + beg[SL], Gl.data(), tc[SL], per_task, tasks);
      const int64_t nt = (int64_t)tasks.size();
      if (nt > 0x7fffffff) return PPR_ERR_RANGE;  // (2^31 slices of one batch: a slice knob far too small)
      const size_t slice_lds = g_lds(pprsubg::sg_table_slots(max_members));
      // ---- the batch's arrays
      size_t tmp_m = 0, tmp_g = 0;
      HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_m, (const int64_t*)nullptr, (int64_t*)nullptr, (int)(Nb + 1), s));
      HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_g, (const int32_t*)nullptr, (int32_t*)nullptr, (int)(Gb + 1), s));
      const size_t tmpb = std::max(tmp_m, tmp_g);
      {
        const int rc = ensure_scratch(&p->d_sgh, &p->sgh_bytes, GBatchDev(nullptr, Nb, Gb, nt, tmpb).bytes);
        if (rc) return rc;
      }
      const GBatchDev h(p->d_sgh, Nb, Gb, nt, tmpb);
      a.nb0 = noff[b0];
      a.ebase = E;
      a.mc = h.mc;
      a.roff = h.roff;
      a.gcnt = h.gcnt;
      a.gbase = h.gbase;
      HIP_OK(hipMemcpyAsync(d.list + b0, list.data(), 4 * (size_t)nb, hipMemcpyHostToDevice, s));
      if (nt) HIP_OK(hipMemcpyAsync(h.tasks, tasks.data(), sizeof(GTask) * (size_t)nt, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemsetAsync(h.mc, 0, 8 * ((size_t)Nb + 1), s));
      HIP_OK(hipMemsetAsync(h.gcnt, 0, 4 * ((size_t)Gb + 1), s));
      const int32_t* dl = d.list + b0;
      // one pass of the walk over the batch: every tier, the same numbering
      auto walk = [&](bool emit) -> int {
        if (tc[0]) {
          const dim3 grid((unsigned)((tc[0] + pprk::G_WPB - 1) / pprk::G_WPB)), block(pprk::G_WPB * WAVE);
          const size_t lds = pprk::G_WPB * g_lds(pprsubg::SG_WAVE_T);
          if (emit) hipLaunchKernelGGL(k_g_wave<true>, grid, block, lds, s, a, dl + beg[0], tc[0]);
          else hipLaunchKernelGGL(k_g_wave<false>, grid, block, lds, s, a, dl + beg[0], tc[0]);
          HIP_OK(hipGetLastError());
        }
        for (int t = WG0; t < SL; t++)
          if (tc[t]) {
            const int T = pprsubg::SG_MIN_T << (t - WG0);
            const dim3 grid((unsigned)tc[t]), block(pprk::G_WG_THREADS);
            if (emit) hipLaunchKernelGGL(k_g_wg<true>, grid, block, g_lds(T), s, a, dl + beg[t], T);
            else hipLaunchKernelGGL(k_g_wg<false>, grid, block, g_lds(T), s, a, dl + beg[t], T);
            HIP_OK(hipGetLastError());
          }
        if (nt) {
          const dim3 grid((unsigned)nt), block(pprk::G_WG_THREADS);
          if (emit) hipLaunchKernelGGL(k_g_slice<true>, grid, block, slice_lds, s, a, (const GTask*)h.tasks);
          else hipLaunchKernelGGL(k_g_slice<false>, grid, block, slice_lds, s, a, (const GTask*)h.tasks);
          HIP_OK(hipGetLastError());
        }
        return PPR_OK;
      };
      // ---- count, scan, rowptr and edge_ptr
      HIP_OK(hipEventRecord(p->ev_m0, s));
      {
        const int rc = walk(false);
        if (rc) return rc;
      }
      size_t tb = tmpb;
      HIP_OK(hipcub::DeviceScan::ExclusiveSum(h.tmp, tb, (const int64_t*)h.mc, h.roff, (int)(Nb + 1), s));
      tb = tmpb;
      HIP_OK(hipcub::DeviceScan::ExclusiveSum(h.tmp, tb, (const int32_t*)h.gcnt, h.gbase, (int)(Gb + 1), s));
      {
        const int64_t nthr = std::max(Nb, nb);
        hipLaunchKernelGGL(k_g_rowptr, dim3((unsigned)((nthr + pprk::G_FLAT_THREADS - 1) / pprk::G_FLAT_THREADS)),
                           dim3(pprk::G_FLAT_THREADS), 0, s, a, b0, nb, Nb);
        HIP_OK(hipGetLastError());
      }
      {
        const int rc = call.lap();
        if (rc) return rc;
      }
      int64_t Eb = 0;
      int32_t Eg = 0;
      HIP_OK(hipMemcpyAsync(&Eb, h.roff + Nb, 8, hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(&Eg, h.gbase + Gb, 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(out.edge_ptr + q0 + b0, d.eptr + b0, 8 * (size_t)nb, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      if (Eb < 0 || Eb > Wb || Eb != (int64_t)Eg) return PPR_ERR_PROBE;  // (cannot happen: both scans count the same hits)
      E += Eb;
      // ---- the capacity check, before any edge is written; then the emit pass
      fits = fits && pprsubg::sg_edges_fit(E, out.edge_cap, idx64);
      if (fits && Eb > 0) {
        HIP_OK(hipEventRecord(p->ev_m0, s));
        const int rc = walk(true);
        if (rc) return rc;
        const int rc2 = call.lap();  // (waits: the batch's arrays are reused by the next one)
        if (rc2) return rc2;
        walked_emit += Wb;
        E_emit += Eb;
      }
    }
  }
  out.node_ptr[S] = N;
  out.edge_ptr[S] = E;
  // a bounded probe that ran out (a sizing error: the planner rules it out)
  {
    const int rc = take_probe_err();
    if (rc) return rc;
  }
  if (st) {
    st->device_ms = call.dev_ms;
    st->edges_walked = walked;
    st->edges = E;
    st->nodes = N;
    st->capped_members = capped;
    st->algo_bytes = 12 * entries + N * (16 + (count_only ? 0 : 2 * isz + (out.scores ? 8 : 0))) + 4 * (walked + walked_emit) +
                     8 * groups + E_emit * (isz + (out.row ? isz : 0) + (out.eid ? 8 : 0));
    st->wave_sources = nwave;
    st->wg_sources = nwg;
    st->slice_sources = nslice;
    st->chunks = (int32_t)std::min<int64_t>((int64_t)cb.size() - 1, INT32_MAX);
  }
  const int rc = pprsubg::sg_capacity(N, E, out.node_cap, out.edge_cap, idx64, count_only);
  if (rc || count_only) return rc;
  // rowptr[N] = E closes the CSR
  if (idx64) {
    HIP_OK(hipMemcpyAsync(reinterpret_cast<int64_t*>(out.rowptr) + N, &E, 8, hipMemcpyHostToDevice, s));
  } else {
    const int32_t e32 = (int32_t)E;
    HIP_OK(hipMemcpyAsync(reinterpret_cast<int32_t*>(out.rowptr) + N, &e32, 4, hipMemcpyHostToDevice, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  return PPR_OK;
}

}  // namespace

extern "C" int ppr_grank_plan_subgraphs(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                                        uint32_t size, int64_t max_deg, uint32_t flags, int64_t node_cap,
                                        int64_t edge_cap, int64_t* node_ptr, int64_t* edge_ptr, void* nodes,
                                        double* scores, void* rowptr, void* col, void* row, int64_t* eid,
                                        ppr_subg_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  const bool plan_ok = p && !p->mc && iterations_run >= 0;
  {
    const int rc = pprsubg::check_subg_args(plan_ok, p ? p->n : 0, S, sources != nullptr, node_ptr && edge_ptr, size, max_deg,
                                            flags, node_cap, edge_cap, nodes != nullptr, rowptr != nullptr, col != nullptr,
                                            scores != nullptr, row != nullptr, eid != nullptr);
    if (rc) return rc;
  }
  if (sources && pprsubg::check_sources(sources, S, p->n)) return PPR_ERR_SOURCE;
  const SubgOut out{node_cap, edge_cap, node_ptr, edge_ptr, nodes, rowptr, col, row, scores, eid};
  return subg_core(p, iterations_run, S, sources, pprsubg::sg_width(size, p->L), max_deg,
                   (flags & PPR_SUBG_ROOT_FIRST) != 0, (flags & PPR_SUBG_IDX64) != 0, out, st);
}
