// rquery.hip -- reverse queries answered from a GRank plan's resident baskets
// (ppr_grank_plan_rquery, include/ppr_hip.h; device code and the semantics: rquery.h).
//
// Host side of one call: every argument check, the factors f_j = w_j / W (W summed in target order
// in fp64), the chunking and the batching of the lists. Knobs, read per call:
//   PPR_R_T          target-table slots T, a power of two 256 .. 8192 (default 8192). A chunk is a run
//                    of consecutive queries with at most 3/4 T postings (so no table can fill, see
//                    rquery.h), PPR_R_CHUNK queries (default 4096) and 2^24 output entries; a single
//                    query with more than 3/4 T targets (6144 at the default) is PPR_ERR_RANGE.
//   PPR_R_PROBE_MAX  a chunk with at most this many postings (and lists of n entries per non-empty
//                    query within E) takes the probe tier; 0 disables it.
//   PPR_R_ENTRIES    E = max(PPR_R_ENTRIES, n) list entries per emit batch (default 2^24).
//   PPR_R_SEG        entries per segment of the list reduction (at least 2 Kq).
// Scan tier, per chunk: the host transposes the chunk's query CSR into a target -> postings CSR and
// builds the image of the target table (the smallest power of two >= 4/3 distinct targets); a count
// pass gives every query's hits, the host groups the queries in order into emit batches whose hits
// sum to at most E (one query's hits are at most n <= E), and one emit pass per batch fills the
// lists. A separate count pass was kept: it reads no score, and it is what bounds the list memory at
// 12 E bytes for any hit counts -- a single pass with worst-case lists would need 12 n bytes per
// query. The reduction levels append at most as many entries again (a segment holds >= 2 Kq).
// The argument checks and the factors are resident_args.h's, the scratch, timing and probe-error
// plumbing resident_call.h's (shared with query.hip and propagate.hip); the table image is built
// with the hash32 the kernels probe it with (hash32.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "resident_call.h"
#include "rquery.h"

namespace {

constexpr int64_t R_CHUNK_DEFAULT = 4096, R_CHUNK_OUT = 1 << 24, R_ENTRIES_DEFAULT = 1 << 24;
constexpr int64_t R_SEG_DEFAULT = 1024, R_PROBE_MAX_DEFAULT = 16;

// device arrays of one chunk (nq queries, np postings), carved from ppr_plan::d_r
struct RChunkDev {
  int64_t* qptr;
  int32_t* targets;
  double* fac;
  uint32_t* tkeys;
  uint32_t* tvals;
  int32_t* tptr;
  int32_t* pq;
  double* pf;
  int32_t* hits;
  int64_t* loff;
  int32_t* lcnt;
  int32_t* ovf;
  int32_t* ovf_cnt;
  unsigned long long* stat;
  int32_t* out_ids;
  double* out_sc;
  int32_t* out_len;
  size_t bytes;
  // nc = counters = nq << lgS
  RChunkDev(unsigned char* base, int64_t nq, int64_t np, int64_t T, int64_t n, int64_t Kq, int64_t nc) {
    Carve c{base};
    qptr = c.take<int64_t>(nq + 1);
    targets = c.take<int32_t>(np);
    fac = c.take<double>(np);
    tkeys = c.take<uint32_t>(T);
    tvals = c.take<uint32_t>(T);
    tptr = c.take<int32_t>(np + 1);
    pq = c.take<int32_t>(np);
    pf = c.take<double>(np);
    hits = c.take<int32_t>(nc * R_CSTRIDE);
    loff = c.take<int64_t>(nc);
    lcnt = c.take<int32_t>(nc * R_CSTRIDE);
    ovf = c.take<int32_t>(n);
    ovf_cnt = c.take<int32_t>(1);
    stat = c.take<unsigned long long>(2);
    out_ids = c.take<int32_t>(nq * Kq);
    out_sc = c.take<double>(nq * Kq);
    out_len = c.take<int32_t>(nq);
    bytes = c.off;
  }
};

}  // namespace

extern "C" int ppr_grank_plan_rquery(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* qptr,
                                     const int32_t* targets, const double* weights, uint32_t Kq, uint32_t flags,
                                     int32_t* out_sources, double* out_scores, int32_t* out_len,
                                     ppr_rquery_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  std::vector<double> fac;  // f_j = w_j / W, W summed in target order
  {
    const int rc = pprres::check_weighted_sets(p && !p->mc && iterations_run >= 0, p ? p->n : 0, Q, qptr, targets,
                                               weights, out_sources && out_scores && out_len, Kq, R_MAX_K, flags,
                                               PPR_RQUERY_EXCLUDE_TARGETS, fac);
    if (rc) return rc;
  }
  const int T = std::max(R_MIN_T, std::min(R_MAX_T, pow2_at_least(env_i64("PPR_R_T", R_MAX_T))));
  const int64_t cap = 3 * (int64_t)T / 4;  // postings of a chunk
  for (int64_t q = 0; q < Q; q++)
    if (qptr[q + 1] - qptr[q] > cap) return PPR_ERR_RANGE;
  if (Q == 0) return PPR_OK;

  const int64_t n = p->n, K = Kq;
  const int64_t chunk_q = std::max<int64_t>(1, env_i64("PPR_R_CHUNK", R_CHUNK_DEFAULT));
  const int64_t probe_max = std::max<int64_t>(0, env_i64("PPR_R_PROBE_MAX", R_PROBE_MAX_DEFAULT));
  const int64_t E = std::max<int64_t>(env_i64("PPR_R_ENTRIES", R_ENTRIES_DEFAULT), n);
  const int64_t SEG = std::min<int64_t>(1 << 30, std::max<int64_t>(env_i64("PPR_R_SEG", R_SEG_DEFAULT), 2 * K));

  ResidentCall call;
  {
    const int rc = call.begin(p, iterations_run);
    if (rc) return rc;
  }
  hipStream_t s = call.s;
  const DevSlab& slab = call.slab;
  const int Kp = pprres::pow2_at_least_k(Kq);
  // row walk geometry (rquery.h k_r_scan)
  const int V = p->L % 4 == 0 ? 4 : 1;
  int lgG = 0;
  while (lgG < 6 && ((int64_t)V << lgG) < (int64_t)p->L) lgG++;
  const int64_t nwin = (n + (WAVE >> lgG) - 1) / (WAVE >> lgG);
  const unsigned scan_grid = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((nwin + R_SCAN_THREADS / WAVE - 1) / (R_SCAN_THREADS / WAVE), 2048));

  {
    int rc = set_lds((const void*)k_r_scan<false, 1>, r_scan_lds(T));
    if (!rc) rc = set_lds((const void*)k_r_scan<true, 1>, r_scan_lds(T));
    if (!rc) rc = set_lds((const void*)k_r_scan<false, 4>, r_scan_lds(T));
    if (!rc) rc = set_lds((const void*)k_r_scan<true, 4>, r_scan_lds(T));
    if (!rc) rc = set_lds((const void*)k_r_ovf<false>, xt_bytes(T));
    if (!rc) rc = set_lds((const void*)k_r_ovf<true>, xt_bytes(T));
    if (!rc) rc = set_lds((const void*)k_r_final, r_final_lds(Kp));
    if (rc) return rc;
  }

  int64_t tot_hits = 0, probe_queries = 0, scan_queries = 0, scans = 0, nchunks = 0, list_entries = 0;
  int64_t sumlen = -1, probe_bytes = 0;

  // Reduce the lists of queries [b0, b1) of the chunk (offset lo[q], hl[q] entries, in the arrays of
  // d_rl) level by level and write their result rows. The lists end at entry `used`; the levels'
  // entries are appended behind. Tasks are uploaded before the timed span.
  std::vector<RSeg> tasks;
  std::vector<int64_t> lvl;  // task range of each level, then the final tasks
  auto plan_reduce = [&](int64_t b0, int64_t b1, const std::vector<int64_t>& lo, const std::vector<int32_t>& hl,
                         int64_t used) -> int64_t {
    tasks.clear();
    lvl.assign(1, 0);
    std::vector<int64_t> off(lo.begin() + b0, lo.begin() + b1);
    std::vector<int64_t> len(b1 - b0);
    for (int64_t i = 0; i < b1 - b0; i++) len[i] = hl[b0 + i];
    for (;;) {
      bool any = false;
      for (int64_t i = 0; i < b1 - b0; i++) {
        if (len[i] <= SEG) continue;
        any = true;
        const int64_t o0 = used;
        for (int64_t a = 0; a < len[i]; a += SEG) {
          const int64_t m = std::min<int64_t>(SEG, len[i] - a);
          tasks.push_back(RSeg{off[i] + a, used, (int32_t)m, (int32_t)(b0 + i)});
          used += std::min<int64_t>(m, K);
        }
        off[i] = o0;
        len[i] = used - o0;
      }
      if (!any) break;
      lvl.push_back((int64_t)tasks.size());
    }
    for (int64_t i = 0; i < b1 - b0; i++) tasks.push_back(RSeg{off[i], 0, (int32_t)len[i], (int32_t)(b0 + i)});
    lvl.push_back((int64_t)tasks.size());
    return used;
  };
  // d_rl: list keys and values (room for `entries`); d_rt: the reduction's tasks
  int32_t* lk = nullptr;
  double* lv = nullptr;
  RSeg* d_tasks = nullptr;
  int64_t reserved = 0;
  auto reserve_lists = [&](int64_t entries) -> int {
    const int rc = ensure_scratch(&p->d_rl, &p->rl_bytes, rnd256(4 * (size_t)entries) + rnd256(8 * (size_t)entries));
    if (rc) return rc;
    Carve cv{p->d_rl};
    lk = cv.take<int32_t>(entries);
    lv = cv.take<double>(entries);
    reserved = entries;
    return PPR_OK;
  };
  auto upload_tasks = [&]() -> int {
    const int rc = ensure_scratch(&p->d_rt, &p->rt_bytes, sizeof(RSeg) * tasks.size());
    if (rc) return rc;
    d_tasks = reinterpret_cast<RSeg*>(p->d_rt);
    HIP_OK(hipMemcpyAsync(d_tasks, tasks.data(), sizeof(RSeg) * tasks.size(), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));  // (tasks is reused by the next batch)
    return PPR_OK;
  };
  auto launch_reduce = [&](const RChunkDev& d) -> int {
    for (size_t l = 0; l + 2 < lvl.size(); l++) {
      const int64_t nt = lvl[l + 1] - lvl[l];
      hipLaunchKernelGGL(k_r_seg, dim3((unsigned)((nt + R_WPB - 1) / R_WPB)), dim3(R_WPB * WAVE), 0, s,
                         d_tasks + lvl[l], nt, lk, lv, (int)Kq);
      HIP_OK(hipGetLastError());
    }
    const int64_t f0 = lvl[lvl.size() - 2], nf = lvl.back() - f0;
    hipLaunchKernelGGL(k_r_final, dim3((unsigned)nf), dim3(WAVE), r_final_lds(Kp), s, d_tasks + f0, lk, lv, (int)Kq, Kp,
                       d.out_ids, d.out_sc, d.out_len);
    HIP_OK(hipGetLastError());
    return PPR_OK;
  };

  std::vector<int64_t> rel, loff, coff;
  std::vector<int32_t> hits, csub, cpad, order, tptr, pq;
  std::vector<uint32_t> tkeys, tvals;
  std::vector<double> pf;
  for (int64_t q0 = 0; q0 < Q;) {
    // ---- the chunk: consecutive queries, postings <= 3/4 T
    int64_t q1 = q0 + 1;
    while (q1 < Q && q1 - q0 < chunk_q && qptr[q1 + 1] - qptr[q0] <= cap && (q1 + 1 - q0) * K <= R_CHUNK_OUT) q1++;
    const int64_t nq = q1 - q0, np = qptr[q1] - qptr[q0], j0 = qptr[q0];
    nchunks++;
    int64_t nonempty = 0;
    for (int64_t q = q0; q < q1; q++) nonempty += qptr[q + 1] > qptr[q];
    const bool probe = np > 0 && np <= probe_max && nonempty * n <= E;
    (probe ? probe_queries : scan_queries) += nq;

    // sub-lists per query (rquery.h R_CSTRIDE): up to 64, about 4096 counters per chunk; one when probing
    int lgS = 0;
    while (!probe && lgS < R_MAX_LGS && (nq << (lgS + 1)) <= 4096) lgS++;
    const int64_t nc = nq << lgS, S = (int64_t)1 << lgS;
    {
      const int rc = ensure_scratch(&p->d_r, &p->r_bytes, RChunkDev(nullptr, nq, np, T, n, K, nc).bytes);
      if (rc) return rc;
    }
    const RChunkDev d(p->d_r, nq, np, T, n, K, nc);
    RArgs a;
    std::memset(&a, 0, sizeof(a));
    a.part = p->d_part; a.sA = call.sA; a.sB = call.sB; a.Kq = (int)Kq; a.exclude = flags & PPR_RQUERY_EXCLUDE_TARGETS;
    a.nq = (int)nq; a.lgS = lgS; a.qptr = d.qptr; a.targets = d.targets; a.fac = d.fac;
    a.tkeys = d.tkeys; a.tvals = d.tvals; a.Tt = 4; a.tptr = d.tptr; a.pq = d.pq; a.pf = d.pf;
    a.hits = d.hits; a.loff = d.loff; a.lcnt = d.lcnt; a.ovf = d.ovf; a.ovf_cnt = d.ovf_cnt; a.stat = d.stat;
    HIP_OK(hipMemsetAsync(d.stat, 0, 16, s));
    hits.assign((size_t)nq, 0);
    loff.assign((size_t)nq, -1);  // per query: the offset of its list
    cpad.resize((size_t)(nc * R_CSTRIDE));

    if (np == 0) {
      // nothing to look up: empty rows
    } else if (probe) {
      rel.resize(nq + 1);
      for (int64_t i = 0; i <= nq; i++) rel[i] = qptr[q0 + i] - j0;
      int64_t used = 0;
      for (int64_t i = 0; i < nq; i++)
        if (rel[i + 1] > rel[i]) { loff[i] = used; used += n; }
      HIP_OK(hipMemcpyAsync(d.qptr, rel.data(), 8 * (size_t)(nq + 1), hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.targets, targets + j0, 4 * (size_t)np, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.fac, fac.data() + j0, 8 * (size_t)np, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.loff, loff.data(), 8 * (size_t)nq, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemsetAsync(d.lcnt, 0, 4 * (size_t)(nc * R_CSTRIDE), s));
      {
        // the lists, and behind them the reduction's levels: a level has at most half its input's
        // entries plus Kq (a segment holds >= 2 Kq), so all levels of a query's list of len entries
        // stay below len + 2 Kq per level, and there are fewer than 32 levels
        const int rc = reserve_lists(2 * used + 64 * K * nonempty);
        if (rc) return rc;
      }
      a.lk = lk; a.lv = lv;
      HIP_OK(hipEventRecord(p->ev_m0, s));
      hipLaunchKernelGGL(k_r_probe, dim3((unsigned)((n + R_PROBE_THREADS - 1) / R_PROBE_THREADS)), dim3(R_PROBE_THREADS), 0,
                         s, slab, a);
      HIP_OK(hipGetLastError());
      {
        const int rc = call.lap();
        if (rc) return rc;
      }
      HIP_OK(hipMemcpyAsync(cpad.data(), d.lcnt, 4 * (size_t)(nc * R_CSTRIDE), hipMemcpyDeviceToHost, s));
      unsigned long long stat[2] = {0, 0};
      HIP_OK(hipMemcpyAsync(stat, d.stat, 16, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      for (int64_t i = 0; i < nq; i++) hits[i] = (int32_t)std::max<int64_t>(0, std::min<int64_t>(cpad[i * R_CSTRIDE], n));
      probe_bytes += 4 * n * np + 4 * (int64_t)stat[1];
    } else {
      // ---- scan tier: target -> postings CSR (postings of a target in query order) and the table image
      order.resize((size_t)np);
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return targets[j0 + x] < targets[j0 + y]; });
      pq.resize((size_t)np);
      pf.resize((size_t)np);
      tptr.clear();
      std::vector<int32_t> dkey;
      {
        int64_t q = q0;
        std::vector<int32_t> qof((size_t)np);
        for (int64_t i = 0; i < np; i++) {
          while (qptr[q + 1] - j0 <= i) q++;
          qof[i] = (int32_t)(q - q0);
        }
        for (int64_t i = 0; i < np; i++) {
          const int32_t t = targets[j0 + order[i]];
          if (i == 0 || t != dkey.back()) { dkey.push_back(t); tptr.push_back((int32_t)i); }
          pq[i] = qof[order[i]];
          pf[i] = fac[j0 + order[i]];
        }
        tptr.push_back((int32_t)np);
      }
      const int64_t D = (int64_t)dkey.size();
      const int Tt = std::max(4, pow2_at_least((4 * D + 2) / 3));  // <= T: D <= 3/4 T
      tkeys.assign((size_t)Tt, 0u);
      tvals.assign((size_t)Tt, 0u);
      for (int64_t i = 0; i < D; i++) {
        uint32_t g = hash32((uint32_t)dkey[i]) & (uint32_t)(Tt - 1) & ~3u;
        for (;;) {  // (ends: the image is at most 3/4 full)
          int e = -1;
          for (int k = 0; k < 4 && e < 0; k++)
            if (tkeys[g + k] == 0u) e = k;
          if (e >= 0) { tkeys[g + e] = (uint32_t)dkey[i] + 1u; tvals[g + e] = (uint32_t)i; break; }
          g = (g + 4u) & (uint32_t)(Tt - 1);
        }
      }
      a.Tt = Tt;
      HIP_OK(hipMemcpyAsync(d.tkeys, tkeys.data(), 4 * (size_t)Tt, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.tvals, tvals.data(), 4 * (size_t)Tt, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.tptr, tptr.data(), 4 * (size_t)(D + 1), hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.pq, pq.data(), 4 * (size_t)np, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(d.pf, pf.data(), 8 * (size_t)np, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemsetAsync(d.hits, 0, 4 * (size_t)(nc * R_CSTRIDE), s));
      HIP_OK(hipMemsetAsync(d.ovf_cnt, 0, 4, s));
      HIP_OK(hipStreamSynchronize(s));
      // overflow table: distinct queries of a row <= min(postings, queries) <= 3/4 of its slots
      const int To = std::max(R_MIN_T, pow2_at_least((4 * std::min<int64_t>(np, nq) + 2) / 3));
      const size_t lds_scan = r_scan_lds(Tt);
      auto scan = [&](bool emit) -> int {
        if (V == 4) {
          if (emit) hipLaunchKernelGGL((k_r_scan<true, 4>), dim3(scan_grid), dim3(R_SCAN_THREADS), lds_scan, s, slab, a, lgG, nwin);
          else hipLaunchKernelGGL((k_r_scan<false, 4>), dim3(scan_grid), dim3(R_SCAN_THREADS), lds_scan, s, slab, a, lgG, nwin);
        } else {
          if (emit) hipLaunchKernelGGL((k_r_scan<true, 1>), dim3(scan_grid), dim3(R_SCAN_THREADS), lds_scan, s, slab, a, lgG, nwin);
          else hipLaunchKernelGGL((k_r_scan<false, 1>), dim3(scan_grid), dim3(R_SCAN_THREADS), lds_scan, s, slab, a, lgG, nwin);
        }
        HIP_OK(hipGetLastError());
        scans++;
        return PPR_OK;
      };
      // ---- count pass
      HIP_OK(hipEventRecord(p->ev_m0, s));
      int rc = scan(false);
      if (!rc) rc = call.lap();
      if (rc) return rc;
      int32_t novf = 0;
      HIP_OK(hipMemcpyAsync(&novf, d.ovf_cnt, 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      novf = (int32_t)std::max<int64_t>(0, std::min<int64_t>(novf, n));
      if (novf) {
        HIP_OK(hipEventRecord(p->ev_m0, s));
        hipLaunchKernelGGL((k_r_ovf<false>), dim3((unsigned)novf), dim3(R_OVF_THREADS), xt_bytes(To), s, slab, a, To);
        HIP_OK(hipGetLastError());
        rc = call.lap();
        if (rc) return rc;
      }
      unsigned long long stat[2] = {0, 0};
      HIP_OK(hipMemcpyAsync(cpad.data(), d.hits, 4 * (size_t)(nc * R_CSTRIDE), hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(stat, d.stat, 16, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      sumlen = (int64_t)stat[0];
      csub.resize((size_t)nc);  // hits per sub-list; a query's hits are their sum (at most n: a row hits once)
      for (int64_t c = 0; c < nc; c++) csub[c] = (int32_t)std::max<int64_t>(0, std::min<int64_t>(cpad[c * R_CSTRIDE], n));
      for (int64_t i = 0; i < nq; i++) {
        int64_t h = 0;
        for (int64_t k = 0; k < S; k++) h += csub[i * S + k];
        if (h > n) return PPR_ERR_PROBE;  // (cannot happen)
        hits[i] = (int32_t)h;
      }
      coff.resize((size_t)nc);
      // ---- emit batches: queries in order, hits summing to at most E
      for (int64_t b0 = 0; b0 < nq;) {
        int64_t b1 = b0, used = 0;
        std::fill(loff.begin(), loff.end(), -1);
        std::fill(coff.begin(), coff.end(), -1);
        while (b1 < nq && (b1 == b0 || used + hits[b1] <= E)) {
          loff[b1] = used;  // the sub-lists of a query lie one behind the other: one list
          for (int64_t k = 0; k < S; k++) { coff[b1 * S + k] = used; used += csub[b1 * S + k]; }
          b1++;
        }
        const int64_t total = plan_reduce(b0, b1, loff, hits, used);
        rc = reserve_lists(total);
        if (!rc) rc = upload_tasks();
        if (rc) return rc;
        a.lk = lk; a.lv = lv;
        HIP_OK(hipMemcpyAsync(d.loff, coff.data(), 8 * (size_t)nc, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemsetAsync(d.lcnt, 0, 4 * (size_t)(nc * R_CSTRIDE), s));
        HIP_OK(hipMemsetAsync(d.ovf_cnt, 0, 4, s));
        HIP_OK(hipStreamSynchronize(s));  // (coff is reused by the next batch)
        HIP_OK(hipEventRecord(p->ev_m0, s));
        rc = scan(true);
        if (rc) return rc;
        if (novf) {  // the same rows overflow in every pass
          hipLaunchKernelGGL((k_r_ovf<true>), dim3((unsigned)novf), dim3(R_OVF_THREADS), xt_bytes(To), s, slab, a, To);
          HIP_OK(hipGetLastError());
        }
        rc = launch_reduce(d);
        if (!rc) rc = call.lap();
        if (rc) return rc;
        list_entries += used;
        b0 = b1;
      }
    }
    if (np == 0 || probe) {  // (the scan tier reduced its batches above)
      int64_t used = 0;
      for (int64_t i = 0; i < nq; i++) used = std::max(used, loff[i] < 0 ? 0 : loff[i] + n);
      for (int64_t i = 0; i < nq; i++)
        if (loff[i] < 0) loff[i] = 0;  // an empty query: no entries
      const int64_t total = plan_reduce(0, nq, loff, hits, used);
      if (np == 0) {
        const int rc0 = reserve_lists(0);
        if (rc0) return rc0;
      }
      if (total > reserved) return PPR_ERR_PROBE;  // (cannot happen: see the reservation above)
      int rc = upload_tasks();
      if (rc) return rc;
      HIP_OK(hipEventRecord(p->ev_m0, s));
      rc = launch_reduce(d);
      if (!rc) rc = call.lap();
      if (rc) return rc;
      for (int64_t i = 0; i < nq; i++) list_entries += hits[i];
    }
    for (int64_t i = 0; i < nq; i++) tot_hits += hits[i];
    HIP_OK(hipMemcpyAsync(out_sources + q0 * K, d.out_ids, 4 * (size_t)(nq * K), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out_scores + q0 * K, d.out_sc, 8 * (size_t)(nq * K), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out_len + q0, d.out_len, 4 * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    q0 = q1;
  }
  // a bounded probe that ran out (a sizing error: the chunking rules it out)
  {
    const int rc = take_probe_err();
    if (rc) return rc;
  }
  if (st) {
    st->device_ms = call.dev_ms;
    st->hits = tot_hits;
    st->algo_bytes = scans * (4 * std::max<int64_t>(sumlen, 0) + 4 * n) + probe_bytes + 32 * list_entries + Q * (12 * K + 4);
    st->probe_queries = probe_queries;
    st->scan_queries = scan_queries;
    st->scans = scans;
    st->chunks = (int32_t)std::min<int64_t>(nchunks, INT32_MAX);
  }
  return PPR_OK;
}
