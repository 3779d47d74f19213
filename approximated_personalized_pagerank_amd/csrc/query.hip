// query.hip -- preference-set queries answered from a GRank plan's resident baskets
// (ppr_grank_plan_query, include/ppr_hip.h; device code and the semantics: query.h).
//
// Host side of one call: every argument check, the seed factors f_i = w_i / W (W summed in seed
// order in fp64) and the chunking. The call is processed in chunks of at most PPR_Q_CHUNK queries
// (default 2^18), 2^22 seeds and 2^24 output entries (a single query larger than that is a chunk of
// its own), so the device scratch cached on the plan stays below ~270 MB for the query arrays and
// outputs plus 2^24 list entries (192 MB) for the range tier, whatever Q is. Phase A plans every
// chunk (k_q_plan) and refuses the call with PPR_ERR_RANGE if a query is too wide for the range
// tier -- before any merge kernel starts; phase B merges chunk by chunk. A query's result does not
// depend on its chunk, its tier or its place in the call.
// The argument checks and the factors are resident_args.h's, the scratch, timing and probe-error
// plumbing resident_call.h's; both are shared with rquery.hip and propagate.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "resident_call.h"
#include "query.h"

namespace {

constexpr int64_t Q_CHUNK_DEFAULT = 1 << 18, Q_CHUNK_SEEDS = 1 << 22, Q_CHUNK_OUT = 1 << 24;
constexpr int64_t Q_BATCH_ENTRIES = 1 << 24, Q_BATCH_TASKS = 1 << 20;

// device arrays of one chunk (nq queries, ns seeds), carved from ppr_plan::d_q
struct ChunkDev {
  int64_t* qptr;
  int32_t* seeds;
  double* fac;
  int32_t* code;
  int64_t* cand;
  int32_t* list;
  int32_t* out_ids;
  double* out_sc;
  int32_t* out_len;
  size_t bytes;
  ChunkDev(unsigned char* base, int64_t nq, int64_t ns, int64_t Kq) {
    Carve c{base};
    qptr = c.take<int64_t>(nq + 1);
    seeds = c.take<int32_t>(ns);
    fac = c.take<double>(ns);
    code = c.take<int32_t>(nq);
    cand = c.take<int64_t>(nq);
    list = c.take<int32_t>(nq);
    out_ids = c.take<int32_t>(nq * Kq);
    out_sc = c.take<double>(nq * Kq);
    out_len = c.take<int32_t>(nq);
    bytes = c.off;
  }
};

}  // namespace

extern "C" int ppr_grank_plan_query(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* qptr,
                                    const int32_t* seeds, const double* weights, uint32_t Kq, uint32_t flags,
                                    int32_t* out_ids, double* out_scores, int32_t* out_len, ppr_query_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  std::vector<double> fac;  // f_i = w_i / W, W summed in seed order
  {
    const int rc = pprres::check_weighted_sets(p && !p->mc && iterations_run >= 0, p ? p->n : 0, Q, qptr, seeds, weights,
                                               out_ids && out_scores && out_len, Kq, Q_MAX_K,
                                               flags, PPR_QUERY_EXCLUDE_SEEDS, fac);
    if (rc) return rc;
  }
  if (Q == 0) return PPR_OK;
  const int64_t NS = qptr[Q];

  // test knobs, read per call
  const int wave_max = (int)std::max<int64_t>(0, std::min<int64_t>(3 * (Q_MIN_T << (Q_WAVE_CLASSES - 1)) / 4,
                                                                   env_i64("PPR_Q_WAVE_MAX", 1536)));
  const int T = std::max(Q_MIN_T, std::min(Q_MAX_T, pow2_at_least(env_i64("PPR_Q_T", Q_MAX_T))));
  const int64_t chunk_q = std::max<int64_t>(1, env_i64("PPR_Q_CHUNK", Q_CHUNK_DEFAULT));

  ResidentCall call;
  {
    const int rc = call.begin(p, iterations_run);
    if (rc) return rc;
  }
  hipStream_t s = call.s;
  const DevSlab& slab = call.slab;
  const int64_t K = Kq;
  const int Kp = pprres::pow2_at_least_k(Kq);

  // chunk boundaries
  std::vector<int64_t> cb{0};
  for (int64_t q = 0; q < Q;) {
    int64_t e = q + 1;
    while (e < Q && e - q < chunk_q && qptr[e + 1] - qptr[q] <= Q_CHUNK_SEEDS && (e + 1 - q) * K <= Q_CHUNK_OUT) e++;
    cb.push_back(e);
    q = e;
  }
  const size_t nchunks = cb.size() - 1;

  std::vector<int64_t> rel;
  auto upload = [&](int64_t q0, int64_t q1, ChunkDev* store) -> int {
    const int64_t nq = q1 - q0, ns = qptr[q1] - qptr[q0];
    const size_t need = ChunkDev(nullptr, nq, ns, K).bytes;
    const int rc = ensure_scratch(&p->d_q, &p->q_bytes, need);
    if (rc) return rc;
    *store = ChunkDev(p->d_q, nq, ns, K);
    rel.resize(nq + 1);
    for (int64_t i = 0; i <= nq; i++) rel[i] = qptr[q0 + i] - qptr[q0];
    HIP_OK(hipMemcpyAsync(store->qptr, rel.data(), 8 * (size_t)(nq + 1), hipMemcpyHostToDevice, s));
    if (ns) {
      HIP_OK(hipMemcpyAsync(store->seeds, seeds + qptr[q0], 4 * (size_t)ns, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(store->fac, fac.data() + qptr[q0], 8 * (size_t)ns, hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipStreamSynchronize(s));  // (rel is reused by the next chunk)
    return PPR_OK;
  };
  auto qargs = [&](const ChunkDev& d) {
    QArgs a;
    a.qptr = d.qptr; a.seeds = d.seeds; a.fac = d.fac; a.part = p->d_part;
    a.sA = call.sA; a.sB = call.sB; a.Kq = (int)Kq; a.exclude = flags & PPR_QUERY_EXCLUDE_SEEDS;
    a.out_ids = d.out_ids; a.out_sc = d.out_sc; a.out_len = d.out_len;
    return a;
  };

  // ---- phase A: plan every chunk
  std::vector<int32_t> code((size_t)Q);
  std::vector<int64_t> cand((size_t)Q);
  ChunkDev cd(nullptr, 0, 0, 1);
  for (size_t c = 0; c < nchunks; c++) {
    const int64_t q0 = cb[c], q1 = cb[c + 1], nq = q1 - q0;
    int rc = upload(q0, q1, &cd);
    if (rc) return rc;
    HIP_OK(hipEventRecord(p->ev_m0, s));
    hipLaunchKernelGGL(k_q_plan, dim3((unsigned)((nq + Q_WPB - 1) / Q_WPB)), dim3(Q_WPB * WAVE), 0, s, slab, qargs(cd),
                       nq, wave_max, T, cd.code, cd.cand);
    HIP_OK(hipGetLastError());
    rc = call.lap();
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(code.data() + q0, cd.code, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(cand.data() + q0, cd.cand, 8 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }
  int64_t C = 0, nwave = 0, nwg = 0, nrange = 0;
  int maxR = 1, wg_lg = 8;
  for (int64_t q = 0; q < Q; q++) {
    const int cq = code[q];
    if (cq < 0) return PPR_ERR_RANGE;  // its fullest key range alone exceeds the table
    C += cand[q];
    if (cq < Q_CODE_WG) nwave++;
    else if (cq < Q_CODE_RANGE) { nwg++; wg_lg = std::max(wg_lg, cq - Q_CODE_WG); }
    else { nrange++; maxR = std::max(maxR, 1 << (cq - Q_CODE_RANGE)); }
  }
  const size_t lds_wave = Q_WPB * q_wave_lds(Q_MIN_T << (Q_WAVE_CLASSES - 1)), lds_wg = q_wave_lds(1 << wg_lg),
               lds_rng = q_wave_lds(T);
  {
    int rc = set_lds((const void*)k_q_wave, lds_wave);
    if (!rc) rc = set_lds((const void*)k_q_wg, lds_wg);
    if (!rc) rc = set_lds((const void*)k_q_range, lds_rng);
    if (!rc) rc = set_lds((const void*)k_q_final, q_final_lds(Kp));
    if (rc) return rc;
  }

  // ---- phase B: merge chunk by chunk
  std::vector<int32_t> list;
  std::vector<QTask> tasks;
  std::vector<int64_t> loff;
  for (size_t c = 0; c < nchunks; c++) {
    const int64_t q0 = cb[c], q1 = cb[c + 1], nq = q1 - q0;
    if (nchunks > 1) {
      const int rc = upload(q0, q1, &cd);
      if (rc) return rc;
    }
    // tier lists (chunk indices, in query order): the wave classes, the workgroup tier by table size
    // (256 .. 8192 slots: a launch's LDS is its own class's table), the range tier
    constexpr int WG0 = Q_WAVE_CLASSES, NWG = 6, RNG = WG0 + NWG, NTIER = RNG + 1;
    int64_t cnt[NTIER] = {}, beg[NTIER + 1] = {};
    auto tier_of = [&](int cq) {
      return cq < Q_CODE_WG ? cq : cq < Q_CODE_RANGE ? WG0 + std::max(0, std::min(NWG - 1, cq - Q_CODE_WG - 8)) : RNG;
    };
    for (int64_t q = q0; q < q1; q++) cnt[tier_of(code[q])]++;
    for (int t = 0; t < NTIER; t++) beg[t + 1] = beg[t] + cnt[t];
    list.resize((size_t)nq);
    {
      int64_t fill[NTIER];
      std::copy(beg, beg + NTIER, fill);
      for (int64_t q = q0; q < q1; q++) list[fill[tier_of(code[q])]++] = (int32_t)(q - q0);
    }
    HIP_OK(hipMemcpyAsync(cd.list, list.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, s));
    // range tier: tasks and list offsets, in batches of bounded list entries
    const int64_t r0 = beg[RNG], nr = cnt[RNG];
    struct Batch { int64_t rq0, rq1, t0, t1; };
    std::vector<Batch> batches;
    tasks.clear();
    loff.assign(1, 0);
    size_t ql_need = 0;
    for (int64_t i = 0; i < nr;) {
      Batch b{i, i, (int64_t)tasks.size(), 0};
      const int64_t o0 = loff.back();
      while (b.rq1 < nr) {
        const int64_t q = q0 + list[r0 + b.rq1];
        const int R = 1 << (code[q] - Q_CODE_RANGE);
        const int64_t ent = std::min<int64_t>((int64_t)R * K, cand[q]);
        if (b.rq1 > b.rq0 && (loff.back() - o0 + ent > Q_BATCH_ENTRIES ||
                              (int64_t)tasks.size() - b.t0 + R > Q_BATCH_TASKS)) break;
        for (int g = 0; g < R; g++) tasks.push_back(QTask{(int32_t)(q - q0), (int32_t)(b.rq1 - b.rq0), g, R});
        loff.push_back(loff.back() + ent);
        b.rq1++;
      }
      b.t1 = (int64_t)tasks.size();
      batches.push_back(b);
      const int64_t nb = b.rq1 - b.rq0, ne = loff.back() - o0;
      ql_need = std::max(ql_need, rnd256(16 * (size_t)(b.t1 - b.t0)) + rnd256(8 * (size_t)(nb + 1)) + rnd256(4 * (size_t)nb) +
                                      rnd256(4 * (size_t)ne) + rnd256(8 * (size_t)ne));
      i = b.rq1;
    }
    if (ql_need) {
      const int rc = ensure_scratch(&p->d_ql, &p->ql_bytes, ql_need);
      if (rc) return rc;
    }
    const QArgs qa = qargs(cd);
    HIP_OK(hipEventRecord(p->ev_m0, s));
    for (int t = 0; t < Q_WAVE_CLASSES; t++)
      if (cnt[t]) {
        const int Tw = Q_MIN_T << t;
        hipLaunchKernelGGL(k_q_wave, dim3((unsigned)((cnt[t] + Q_WPB - 1) / Q_WPB)), dim3(Q_WPB * WAVE),
                           Q_WPB * q_wave_lds(Tw), s, slab, qa, cd.list + beg[t], cnt[t], Tw);
        HIP_OK(hipGetLastError());
      }
    for (int t = WG0; t < RNG; t++)
      if (cnt[t]) {
        const int Tg = Q_MIN_T << (t - WG0);
        hipLaunchKernelGGL(k_q_wg, dim3((unsigned)cnt[t]), dim3(Q_WG_THREADS), q_wave_lds(Tg), s, slab, qa,
                           cd.list + beg[t], Tg);
        HIP_OK(hipGetLastError());
      }
    {
      const int rc = call.lap();
      if (rc) return rc;
    }
    std::vector<int64_t> boff;
    for (const Batch& b : batches) {  // (each batch's tasks are uploaded outside its timed span)
      const int64_t nb = b.rq1 - b.rq0, nt = b.t1 - b.t0, o0 = loff[b.rq0], ne = loff[b.rq1] - o0;
      Carve cv{p->d_ql};
      QTask* d_tasks = cv.take<QTask>(nt);
      int64_t* d_off = cv.take<int64_t>(nb + 1);
      QLists ql;
      ql.cnt = cv.take<int32_t>(nb);
      ql.k = cv.take<int32_t>(ne);
      ql.v = cv.take<double>(ne);
      ql.off = d_off;
      boff.resize(nb + 1);
      for (int64_t i = 0; i <= nb; i++) boff[i] = loff[b.rq0 + i] - o0;
      HIP_OK(hipMemcpyAsync(d_tasks, tasks.data() + b.t0, sizeof(QTask) * (size_t)nt, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d_off, boff.data(), 8 * (size_t)(nb + 1), hipMemcpyHostToDevice, s));
      HIP_OK(hipMemsetAsync(ql.cnt, 0, 4 * (size_t)nb, s));
      HIP_OK(hipStreamSynchronize(s));  // (boff is reused by the next batch)
      HIP_OK(hipEventRecord(p->ev_m0, s));
      hipLaunchKernelGGL(k_q_range, dim3((unsigned)nt), dim3(Q_WG_THREADS), lds_rng, s, slab, qa, d_tasks, T, ql);
      HIP_OK(hipGetLastError());
      hipLaunchKernelGGL(k_q_final, dim3((unsigned)nb), dim3(WAVE), q_final_lds(Kp), s, qa, cd.list + r0 + b.rq0, ql, Kp);
      HIP_OK(hipGetLastError());
      const int rc = call.lap();
      if (rc) return rc;
    }
    HIP_OK(hipMemcpyAsync(out_ids + q0 * K, cd.out_ids, 4 * (size_t)(nq * K), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out_scores + q0 * K, cd.out_sc, 8 * (size_t)(nq * K), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out_len + q0, cd.out_len, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }
  // a bounded probe that ran out (a sizing error: the planner rules it out)
  {
    const int rc = take_probe_err();
    if (rc) return rc;
  }
  if (st) {
    st->device_ms = call.dev_ms;
    st->candidates = C;
    st->algo_bytes = 8 * NS + 12 * C + Q * (12 * K + 4);
    st->wave_queries = nwave;
    st->wg_queries = nwg;
    st->range_queries = nrange;
    st->max_ranges = maxR;
  }
  return PPR_OK;
}
