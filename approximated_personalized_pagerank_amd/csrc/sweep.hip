// sweep.hip -- sweep-cut local clustering from a GRank plan's resident baskets
// (ppr_grank_plan_sweep, ppr_grank_plan_sweep_vectors; include/ppr_hip.h; device code: sweep.h;
// host planning and the refusals: sweep_plan.h).
//
// Host side of one call: every argument check, the chunks, the tier lists of a chunk and the slice
// tasks. Knobs, read per call (no result depends on them):
//   PPR_SW_WAVE_MAX  a source whose walk has at most this many edges (and at most 192 members) is
//                    answered by one wave (default 2048; 0: no source goes to the wave tier)
//   PPR_SW_WG_MAX    ... at most this many edges by one workgroup (default 2^17; 0: none)
//   PPR_SW_SLICE     edges per (source, slice) workgroup beyond that (default 2^15, at least 64)
//   PPR_SW_CHUNK     sources per chunk (default 2^15; a chunk also holds at most 2^22 row entries), so
//                    that the scratch cached on the plan does not grow with S
// Per chunk: k_s_plan orders every row and gives the verdicts, the host sorts the chunk's sources into
// tier lists, k_s_wave / k_s_wg (one launch per table size) answer theirs in place, the slice tier
// runs in batches of bounded histogram rows (k_s_slice, k_s_final). A source's result does not depend
// on its chunk, its tier or its place in the call.
// The slot rule is resident_args.h's, the scratch and timing plumbing resident_call.h's; both are
// shared with query.hip, rquery.hip and propagate.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "resident_call.h"
#include "sweep.h"

namespace {

using pprsweep::SBatch;
using pprsweep::STask;

struct SweepIn {         // the rows of a call
  bool vec;
  int64_t rows;
  const int32_t* sources;  // resident rows (null: row i is source i)
  const int32_t* ids;      // vectors
  const double* scores;
  const int32_t* lens;
  int64_t row_width;       // L or width_in
};
struct SweepOut {
  int32_t *order, *swept, *size;
  int64_t *cut, *vol;
  double* phi;
  int64_t *prof_cut, *prof_vol;
};

// device arrays of one chunk of nq rows, carved from ppr_plan::d_sw
struct ChunkDev {
  int32_t *src, *vids, *vlen;
  double* vsc;
  int32_t *order, *swept, *code, *rlen, *list, *size;
  int64_t *volp, *W, *cut, *vol, *prof_cut;
  double* phi;
  size_t bytes;
  ChunkDev(unsigned char* base, int64_t nq, int64_t width, bool vec, int64_t row_width, bool prof) {
    Carve c{base};
    const size_t q = (size_t)std::max<int64_t>(nq, 1), e = q * (size_t)std::max<int64_t>(width, 1);
    const size_t ve = vec ? q * (size_t)std::max<int64_t>(row_width, 1) : 1;
    src = c.take<int32_t>(q);
    vids = c.take<int32_t>(ve);
    vsc = c.take<double>(ve);
    vlen = c.take<int32_t>(q);
    order = c.take<int32_t>(e);
    volp = c.take<int64_t>(e);
    prof_cut = c.take<int64_t>(prof ? e : 1);
    swept = c.take<int32_t>(q);
    W = c.take<int64_t>(q);
    code = c.take<int32_t>(q);
    rlen = c.take<int32_t>(q);
    list = c.take<int32_t>(q);
    size = c.take<int32_t>(q);
    cut = c.take<int64_t>(q);
    vol = c.take<int64_t>(q);
    phi = c.take<double>(q);
    bytes = c.off;
  }
};

int sweep_core(ppr_plan* p, int32_t iterations_run, const SweepIn& in, uint32_t min_size, int64_t width,
               int64_t max_vol, const SweepOut& out, ppr_sweep_stats* st) {
  const int64_t S = in.rows;
  if (S == 0) return PPR_OK;
  const bool prof = out.prof_cut != nullptr;
  if (max_vol == 0) max_vol = p->m / 2;

  // test knobs, read per call
  const int64_t wave_max = pprsweep::clamp_wave_max(env_i64("PPR_SW_WAVE_MAX", pprsweep::SW_WAVE_MAX_DEFAULT));
  const int64_t wg_max = pprsweep::clamp_wg_max(env_i64("PPR_SW_WG_MAX", pprsweep::SW_WG_MAX_DEFAULT));
  const int64_t slice = pprsweep::clamp_slice(env_i64("PPR_SW_SLICE", pprsweep::SW_SLICE_DEFAULT));
  const int64_t chunk_rows = std::max<int64_t>(1, env_i64("PPR_SW_CHUNK", pprsweep::SW_CHUNK_DEFAULT));

  ResidentCall call;
  {
    const int rc = call.begin(p, in.vec ? 0 : iterations_run);
    if (rc) return rc;
  }
  hipStream_t s = call.s;
  int Lp = WAVE;
  while (Lp < in.row_width) Lp <<= 1;
  const int plan_wpb = Lp <= 1024 ? pprk::S_WPB : 1;
  const bool hk = p->hot_n > 0;
  {
    int rc = set_lds((const void*)k_s_wg, s_lds(pprsweep::SW_MAX_T));
    if (!rc) rc = set_lds((const void*)k_s_slice, s_lds(pprsweep::SW_MAX_T));
    if (rc) return rc;
  }

  const std::vector<int64_t> cb =
      pprsweep::cut_chunks(S, std::max(width, in.row_width), chunk_rows, pprsweep::SW_CHUNK_ENTRIES);
  std::vector<int32_t> code, rlen, swept, list;
  std::vector<int64_t> W, Wl;
  std::vector<STask> tasks;
  std::vector<SBatch> batches;
  int64_t edges = 0, entries = 0, nwave = 0, nwg = 0, nslice = 0;
  for (size_t c = 0; c + 1 < cb.size(); c++) {
    const int64_t q0 = cb[c], q1 = cb[c + 1], nq = q1 - q0;
    {
      const int rc = ensure_scratch(&p->d_sw, &p->sw_bytes, ChunkDev(nullptr, nq, width, in.vec, in.row_width, prof).bytes);
      if (rc) return rc;
    }
    const ChunkDev d(p->d_sw, nq, width, in.vec, in.row_width, prof);
    SArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src_base = q0;
    a.part = p->d_part;
    a.sA = call.sA;
    a.sB = call.sB;
    a.width_in = (int)in.row_width;
    a.rp = p->d_rp;
    a.colx = p->d_colx;
    a.n = p->n;
    a.m = p->m;
    a.width = (int)width;
    a.min_size = (int)min_size;
    a.max_vol = max_vol;
    a.order = d.order; a.volp = d.volp; a.swept = d.swept; a.W = d.W; a.code = d.code; a.rlen = d.rlen;
    a.size = d.size; a.cut = d.cut; a.vol = d.vol; a.phi = d.phi;
    a.prof_cut = prof ? d.prof_cut : nullptr;
    if (in.vec) {
      const size_t ne = (size_t)nq * (size_t)in.row_width;
      if (ne) {
        HIP_OK(hipMemcpyAsync(d.vids, in.ids + q0 * in.row_width, 4 * ne, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(d.vsc, in.scores + q0 * in.row_width, 8 * ne, hipMemcpyHostToDevice, s));
      }
      HIP_OK(hipMemcpyAsync(d.vlen, in.lens + q0, 4 * (size_t)nq, hipMemcpyHostToDevice, s));
      a.vids = d.vids; a.vsc = d.vsc; a.vlen = d.vlen;
    } else if (in.sources) {
      HIP_OK(hipMemcpyAsync(d.src, in.sources + q0, 4 * (size_t)nq, hipMemcpyHostToDevice, s));
      a.src = d.src;
    }
    // ---- the rows in order, the verdicts
    {
      const dim3 grid((unsigned)((nq + plan_wpb - 1) / plan_wpb)), block(plan_wpb * WAVE);
      const size_t lds = plan_wpb * s_plan_lds(Lp);
      HIP_OK(hipEventRecord(p->ev_m0, s));
      if (in.vec) hipLaunchKernelGGL((k_s_plan<true, false>), grid, block, lds, s, call.slab, a, nq, Lp, wave_max, wg_max);
      else if (hk) hipLaunchKernelGGL((k_s_plan<false, true>), grid, block, lds, s, call.slab, a, nq, Lp, wave_max, wg_max);
      else hipLaunchKernelGGL((k_s_plan<false, false>), grid, block, lds, s, call.slab, a, nq, Lp, wave_max, wg_max);
      HIP_OK(hipGetLastError());
      const int rc = call.lap();
      if (rc) return rc;
    }
    code.resize((size_t)nq); rlen.resize((size_t)nq); swept.resize((size_t)nq); W.resize((size_t)nq);
    HIP_OK(hipMemcpyAsync(code.data(), d.code, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(rlen.data(), d.rlen, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(swept.data(), d.swept, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(W.data(), d.W, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    // ---- tier lists (chunk indices, in source order): wave | workgroup by table size | slices
    constexpr int WG0 = 1, NWG = 6, SL = WG0 + NWG, NTIER = SL + 1;
    int64_t cnt[NTIER] = {}, beg[NTIER + 1] = {};
    auto tier_of = [&](int cq) {
      if (cq == pprsweep::SW_CODE_WAVE) return 0;
      if (cq >= pprsweep::SW_CODE_SLICE) return SL;
      return WG0 + std::max(0, std::min(NWG - 1, cq - pprsweep::SW_CODE_WG - 8));
    };
    for (int64_t q = 0; q < nq; q++) {
      cnt[tier_of(code[q])]++;
      edges += W[q];
      entries += rlen[q];
    }
    for (int t = 0; t < NTIER; t++) beg[t + 1] = beg[t] + cnt[t];
    list.resize((size_t)nq);
    {
      int64_t fill[NTIER];
      std::copy(beg, beg + NTIER, fill);
      for (int64_t q = 0; q < nq; q++) list[fill[tier_of(code[q])]++] = (int32_t)q;
    }
    nwave += cnt[0];
    nslice += cnt[SL];
    nwg += nq - cnt[0] - cnt[SL];
    HIP_OK(hipMemcpyAsync(d.list, list.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(p->ev_m0, s));
    if (cnt[0]) {
      hipLaunchKernelGGL(k_s_wave, dim3((unsigned)((cnt[0] + pprk::S_WPB - 1) / pprk::S_WPB)), dim3(pprk::S_WPB * WAVE),
                         pprk::S_WPB * s_lds(pprsweep::SW_WAVE_T), s, a, d.list + beg[0], cnt[0]);
      HIP_OK(hipGetLastError());
    }
    for (int t = WG0; t < SL; t++)
      if (cnt[t]) {
        const int T = pprsweep::SW_MIN_T << (t - WG0);
        hipLaunchKernelGGL(k_s_wg, dim3((unsigned)cnt[t]), dim3(pprk::S_WG_THREADS), s_lds(T), s, a, d.list + beg[t], T);
        HIP_OK(hipGetLastError());
      }
    {
      const int rc = call.lap();
      if (rc) return rc;
    }
    // ---- the slice tier, in batches of bounded histogram rows
    if (cnt[SL]) {
      Wl.resize((size_t)cnt[SL]);
      int max_sw = 0;
      for (int64_t i = 0; i < cnt[SL]; i++) {
        const int32_t q = list[beg[SL] + i];
        Wl[i] = W[q];
        max_sw = std::max(max_sw, swept[q]);
      }
      pprsweep::cut_slices(list.data() + beg[SL], Wl.data(), cnt[SL], slice,
                           std::max<int64_t>(1, pprsweep::SW_BATCH_ENTRIES / std::max<int64_t>(width, 1)), tasks, batches);
      const size_t lds = s_lds(pprsweep::sw_table_slots(max_sw));
      for (const SBatch& b : batches) {
        const int64_t nt = b.t1 - b.t0, nr = b.r1 - b.r0;
        if (nt > 0x7fffffff) return PPR_ERR_RANGE;  // (2^31 slices of one batch: a slice knob far too small)
        const int rc = ensure_scratch(&p->d_swh, &p->swh_bytes,
                                      rnd256(sizeof(STask) * (size_t)nt) + rnd256(8 * (size_t)nr * (size_t)width));
        if (rc) return rc;
        Carve cv{p->d_swh};
        STask* d_tasks = cv.take<STask>((size_t)nt);
        unsigned long long* gh = cv.take<unsigned long long>((size_t)nr * (size_t)width);
        HIP_OK(hipMemcpyAsync(d_tasks, tasks.data() + b.t0, sizeof(STask) * (size_t)nt, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemsetAsync(gh, 0, 8 * (size_t)nr * (size_t)width, s));
        HIP_OK(hipEventRecord(p->ev_m0, s));
        hipLaunchKernelGGL(k_s_slice, dim3((unsigned)nt), dim3(pprk::S_WG_THREADS), lds, s, a, (const STask*)d_tasks, gh);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(k_s_final, dim3((unsigned)nr), dim3(WAVE), 0, s, a, d.list + beg[SL] + b.r0,
                           (const unsigned long long*)gh);
        HIP_OK(hipGetLastError());
        const int rc2 = call.lap();  // (waits: the batch's arrays are reused by the next one)
        if (rc2) return rc2;
      }
    }
    // ---- the chunk's results
    const size_t ne = (size_t)nq * (size_t)width;
    HIP_OK(hipMemcpyAsync(out.order + q0 * width, d.order, 4 * ne, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out.swept + q0, d.swept, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out.size + q0, d.size, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out.cut + q0, d.cut, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out.vol + q0, d.vol, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out.phi + q0, d.phi, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    if (prof) {
      HIP_OK(hipMemcpyAsync(out.prof_cut + q0 * width, d.prof_cut, 8 * ne, hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(out.prof_vol + q0 * width, d.volp, 8 * ne, hipMemcpyDeviceToHost, s));
    }
    HIP_OK(hipStreamSynchronize(s));
  }
  // a bounded probe that ran out (a sizing error: the planner rules it out)
  {
    const int rc = take_probe_err();
    if (rc) return rc;
  }
  if (st) {
    st->device_ms = call.dev_ms;
    st->edges = edges;
    st->algo_bytes = 28 * entries + 4 * edges + S * (4 * width + 36) + (prof ? 16 * S * width : 0);
    st->wave_sources = nwave;
    st->wg_sources = nwg;
    st->slice_sources = nslice;
    st->chunks = (int32_t)std::min<int64_t>((int64_t)cb.size() - 1, INT32_MAX);
  }
  return PPR_OK;
}

}  // namespace

extern "C" int ppr_grank_plan_sweep(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                                    uint32_t min_size, uint32_t max_size, int64_t max_vol, uint32_t flags,
                                    int32_t* out_order, int32_t* out_swept, int32_t* out_size, int64_t* out_cut,
                                    int64_t* out_vol, double* out_phi, int64_t* prof_cut, int64_t* prof_vol,
                                    ppr_sweep_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  const bool plan_ok = p && !p->mc && iterations_run >= 0;
  {
    const int rc = pprsweep::check_sweep_args(plan_ok, p ? p->n : 0, p ? p->m : 0, S, sources != nullptr, false,
                                              p ? (int64_t)p->L : 0, min_size, max_size, max_vol, flags,
                                              out_order && out_swept && out_size && out_cut && out_vol && out_phi,
                                              prof_cut != nullptr, prof_vol != nullptr);
    if (rc) return rc;
  }
  if (sources && pprsweep::check_sources(sources, S, p->n)) return PPR_ERR_SOURCE;
  const SweepIn in{false, S, sources, nullptr, nullptr, nullptr, (int64_t)p->L};
  const SweepOut out{out_order, out_swept, out_size, out_cut, out_vol, out_phi, prof_cut, prof_vol};
  return sweep_core(p, iterations_run, in, min_size, pprsweep::sweep_width(max_size, p->L, false), max_vol, out, st);
}

extern "C" int ppr_grank_plan_sweep_vectors(ppr_plan* p, int64_t R, int32_t width_in, const int32_t* ids,
                                            const double* scores, const int32_t* lens, uint32_t min_size,
                                            uint32_t max_size, int64_t max_vol, uint32_t flags, int32_t* out_order,
                                            int32_t* out_swept, int32_t* out_size, int64_t* out_cut, int64_t* out_vol,
                                            double* out_phi, int64_t* prof_cut, int64_t* prof_vol,
                                            ppr_sweep_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  {
    const int rc = pprsweep::check_sweep_args(p && !p->mc, p ? p->n : 0, p ? p->m : 0, R, ids && scores && lens, true,
                                              width_in, min_size, max_size, max_vol, flags,
                                              out_order && out_swept && out_size && out_cut && out_vol && out_phi,
                                              prof_cut != nullptr, prof_vol != nullptr);
    if (rc) return rc;
  }
  {
    const int rc = pprsweep::check_vectors(R, width_in, ids, scores, lens, p->n);
    if (rc) return rc;
  }
  const SweepIn in{true, R, nullptr, ids, scores, lens, (int64_t)width_in};
  const SweepOut out{out_order, out_swept, out_size, out_cut, out_vol, out_phi, prof_cut, prof_vol};
  return sweep_core(p, 0, in, min_size, pprsweep::sweep_width(max_size, width_in, true), max_vol, out, st);
}
