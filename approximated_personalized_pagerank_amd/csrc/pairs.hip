// pairs.hip -- node-pair scores from a GRank plan's resident baskets (ppr_grank_plan_pairs;
// include/ppr_hip.h; device code: pairs.h; host planning, the refusals and the byte accounting:
// pairs_plan.h).
//
// Host side of one call: every argument check, the chunks, a chunk's uploads, its tasks by tier, the
// launches of its class and the downloads. Knobs, read per call (no result depends on them):
//   PPR_PR_WAVE_MAX  a group of at most this many candidates is answered by one wave (default 16;
//                    0: no group goes to the wave tier)
//   PPR_PR_SPLIT     a group of more candidates than this is cut into workgroup tasks of this many
//                    (default 1024, at least 1)
//   PPR_PR_CHUNK     groups per chunk (default 2^15; a chunk also holds at most 2^21 pairs and, when
//                    the lookup class ranks, 2^22 rank entries), so that the scratch cached on the plan
//                    does not grow with Q or P
//   PPR_PR_SEARCH    the overlap kernel's search of the LDS segment: 0 by the row width (bisection from
//                    L = 512 on), 1 linear, 2 bisection
// The slot rule is resident_args.h's, the scratch and timing plumbing resident_call.h's; both are
// shared with query.hip, rquery.hip, propagate.hip, sweep.hip and subgraph.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "resident_call.h"
#include "pairs.h"

namespace {

using pprpairs::PChunk;
using pprpairs::PTask;

struct PairsOut {
  double *fwd, *bwd;
  uint8_t* hit;
  int32_t *rank, *common;
  double* dot;
  int32_t *slen, *clen;
};

// device arrays of one chunk of G groups and P pairs, carved from ppr_plan::d_pr
struct PChunkDev {
  int32_t *src, *cand, *pg, *slen;
  double *fwd, *bwd, *dot;
  int32_t *rank, *common, *clen;
  uint8_t* hit;
  uint16_t* rankbuf;
  PTask* tasks;
  unsigned long long* stat;
  size_t bytes;
  PChunkDev(unsigned char* base, int64_t G, int64_t P, int64_t nt, int64_t L, uint32_t outs, bool lookup) {
    Carve c{base};
    const size_t g = (size_t)std::max<int64_t>(G, 1), p = (size_t)std::max<int64_t>(P, 1);
    auto want = [&](uint32_t bit) { return (outs & bit) ? p : (size_t)1; };
    stat = c.take<unsigned long long>(8);
    src = c.take<int32_t>(g);
    slen = c.take<int32_t>(g);
    cand = c.take<int32_t>(p);
    pg = c.take<int32_t>(lookup ? p : 1);
    fwd = c.take<double>(want(pprpairs::PR_FWD));
    bwd = c.take<double>(want(pprpairs::PR_BWD));
    dot = c.take<double>(want(pprpairs::PR_DOT));
    rank = c.take<int32_t>(want(pprpairs::PR_RANK));
    common = c.take<int32_t>(want(pprpairs::PR_COMMON));
    clen = c.take<int32_t>(want(pprpairs::PR_CLEN));
    hit = c.take<uint8_t>(want(pprpairs::PR_HIT));
    rankbuf = c.take<uint16_t>(lookup && (outs & pprpairs::PR_RANK) ? g * (size_t)L : 1);
    tasks = c.take<PTask>((size_t)std::max<int64_t>(nt, 1));
    bytes = c.off;
  }
};

template <bool HK>
int pairs_chunk(ppr_plan* p, ResidentCall& call, const PChunk& ck, const int64_t* gptr, const int32_t* sources,
                const int32_t* cands, uint32_t outs, int cls, const PairsOut& out, int64_t wave_max, int64_t split,
                bool binary, pprpairs::PCount& cnt, int64_t tiers[3]) {
  hipStream_t s = call.s;
  const int64_t G = ck.q1 - ck.q0, P = ck.j1 - ck.j0;
  const bool lookup = cls == pprpairs::PR_LOOKUP;
  const bool ranks = (outs & pprpairs::PR_RANK) != 0;
  int Lp = WAVE;
  while (Lp < (int)p->L) Lp <<= 1;
  std::vector<PTask> wave, wg;
  std::vector<int32_t> pg;
  if (!lookup) {
    pprpairs::cut_tasks(ck, gptr, wave_max, split, wave, wg, tiers);
  } else if (P > 0) {
    pg.resize((size_t)P);
    for (int64_t q = ck.q0; q < ck.q1; q++)
      for (int64_t j = std::max(gptr[q], ck.j0); j < std::min(gptr[q + 1], ck.j1); j++) pg[(size_t)(j - ck.j0)] = (int32_t)(q - ck.q0);
  }
  const int64_t nw = (int64_t)wave.size(), nt = nw + (int64_t)wg.size();
  {
    const int rc = ensure_scratch(&p->d_pr, &p->pr_bytes, PChunkDev(nullptr, G, P, nt, p->L, outs, lookup).bytes);
    if (rc) return rc;
  }
  const PChunkDev d(p->d_pr, G, P, nt, p->L, outs, lookup);
  PArgs a;
  std::memset(&a, 0, sizeof(a));
  a.part = p->d_part;
  a.sA = call.sA;
  a.sB = call.sB;
  a.outs = outs;
  a.binary = binary ? 1 : 0;
  a.Lp = Lp;
  a.src = d.src;
  a.cand = d.cand;
  a.pg = d.pg;
  a.rankbuf = d.rankbuf;
  a.fwd = (outs & pprpairs::PR_FWD) ? d.fwd : nullptr;
  a.bwd = (outs & pprpairs::PR_BWD) ? d.bwd : nullptr;
  a.dot = (outs & pprpairs::PR_DOT) ? d.dot : nullptr;
  a.hit = (outs & pprpairs::PR_HIT) ? d.hit : nullptr;
  a.rank = ranks ? d.rank : nullptr;
  a.common = (outs & pprpairs::PR_COMMON) ? d.common : nullptr;
  a.clen = (outs & pprpairs::PR_CLEN) ? d.clen : nullptr;
  a.stat = d.stat;
  HIP_OK(hipMemsetAsync(d.stat, 0, 8 * sizeof(unsigned long long), s));
  HIP_OK(hipMemcpyAsync(d.src, sources + ck.q0, 4 * (size_t)G, hipMemcpyHostToDevice, s));
  if (P) HIP_OK(hipMemcpyAsync(d.cand, cands + ck.j0, 4 * (size_t)P, hipMemcpyHostToDevice, s));
  if (lookup && P) HIP_OK(hipMemcpyAsync(d.pg, pg.data(), 4 * (size_t)P, hipMemcpyHostToDevice, s));
  if (nw) HIP_OK(hipMemcpyAsync(d.tasks, wave.data(), sizeof(PTask) * (size_t)nw, hipMemcpyHostToDevice, s));
  if (nt > nw) HIP_OK(hipMemcpyAsync(d.tasks + nw, wg.data(), sizeof(PTask) * (size_t)(nt - nw), hipMemcpyHostToDevice, s));
  HIP_OK(hipEventRecord(p->ev_m0, s));
  if (outs & pprpairs::PR_SLEN) {
    hipLaunchKernelGGL(k_p_len<HK>, dim3((unsigned)((G + pprk::P_LEN_WPB - 1) / pprk::P_LEN_WPB)), dim3(pprk::P_LEN_WPB * WAVE), 0,
                       s, call.slab, a, (const int32_t*)d.src, G, d.slen, 3);
    HIP_OK(hipGetLastError());
  }
  if (lookup && P) {
    if (outs & pprpairs::PR_CLEN) {
      hipLaunchKernelGGL(k_p_len<HK>, dim3((unsigned)((P + pprk::P_LEN_WPB - 1) / pprk::P_LEN_WPB)), dim3(pprk::P_LEN_WPB * WAVE),
                         0, s, call.slab, a, (const int32_t*)d.cand, P, d.clen, 4);
      HIP_OK(hipGetLastError());
    }
    if (ranks) {
      hipLaunchKernelGGL(k_p_rank<HK>, dim3((unsigned)G), dim3(WAVE), pprk::p_lds((int)p->L, Lp, true), s, call.slab, a);
      HIP_OK(hipGetLastError());
      cnt.ranked_groups += G;
    }
    hipLaunchKernelGGL(k_p_look<HK>, dim3((unsigned)((P + pprk::P_LOOK_THREADS - 1) / pprk::P_LOOK_THREADS)),
                       dim3(pprk::P_LOOK_THREADS), 0, s, call.slab, a, P);
    HIP_OK(hipGetLastError());
  } else if (!lookup) {
    const size_t lds = pprk::p_lds((int)p->L, Lp, ranks);
    if (nw) {
      hipLaunchKernelGGL((k_p_ovl<HK, 1>), dim3((unsigned)nw), dim3(WAVE), lds, s, call.slab, a, (const PTask*)d.tasks);
      HIP_OK(hipGetLastError());
    }
    if (nt > nw) {
      hipLaunchKernelGGL((k_p_ovl<HK, pprk::P_WG_WAVES>), dim3((unsigned)(nt - nw)), dim3(pprk::P_WG_THREADS), lds, s, call.slab, a,
                         (const PTask*)(d.tasks + nw));
      HIP_OK(hipGetLastError());
    }
  }
  {
    const int rc = call.lap();
    if (rc) return rc;
  }
  // ---- the chunk's results and counters
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(st, d.stat, sizeof(st), hipMemcpyDeviceToHost, s));
  if (out.slen) HIP_OK(hipMemcpyAsync(out.slen + ck.q0, d.slen, 4 * (size_t)G, hipMemcpyDeviceToHost, s));
  if (P) {
    if (out.fwd) HIP_OK(hipMemcpyAsync(out.fwd + ck.j0, d.fwd, 8 * (size_t)P, hipMemcpyDeviceToHost, s));
    if (out.bwd) HIP_OK(hipMemcpyAsync(out.bwd + ck.j0, d.bwd, 8 * (size_t)P, hipMemcpyDeviceToHost, s));
    if (out.dot) HIP_OK(hipMemcpyAsync(out.dot + ck.j0, d.dot, 8 * (size_t)P, hipMemcpyDeviceToHost, s));
    if (out.hit) HIP_OK(hipMemcpyAsync(out.hit + ck.j0, d.hit, (size_t)P, hipMemcpyDeviceToHost, s));
    if (out.rank) HIP_OK(hipMemcpyAsync(out.rank + ck.j0, d.rank, 4 * (size_t)P, hipMemcpyDeviceToHost, s));
    if (out.common) HIP_OK(hipMemcpyAsync(out.common + ck.j0, d.common, 4 * (size_t)P, hipMemcpyDeviceToHost, s));
    if (out.clen) HIP_OK(hipMemcpyAsync(out.clen + ck.j0, d.clen, 4 * (size_t)P, hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  cnt.tasks += lookup ? 0 : nt;
  cnt.task_entries += (int64_t)st[0];
  cnt.cand_entries += (int64_t)st[1];
  cnt.hits += (int64_t)st[2];
  cnt.fwd_hits += (int64_t)st[5];
  cnt.slen_entries += (int64_t)st[3];
  cnt.clen_entries += (int64_t)st[4];
  return PPR_OK;
}

template <bool HK>
int set_pairs_lds(size_t lds) {
  int rc = set_lds((const void*)k_p_rank<HK>, lds);
  if (!rc) rc = set_lds((const void*)(k_p_ovl<HK, 1>), lds);
  if (!rc) rc = set_lds((const void*)(k_p_ovl<HK, pprk::P_WG_WAVES>), lds);
  return rc;
}

int pairs_core(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* gptr, const int32_t* sources,
               const int32_t* cands, uint32_t outs, const PairsOut& out, ppr_pairs_stats* st) {
  const int64_t P = gptr[Q];
  const int cls = pprpairs::pr_class(outs);
  // nothing to launch: no group, or no pair and no per-group output
  if (Q == 0 || (P == 0 && !(outs & pprpairs::PR_SLEN))) {
    if (st) {
      pprpairs::PCount none;
      none.groups = Q;
      st->groups = Q;
      st->algo_bytes = pprpairs::pr_algo_bytes(cls, outs, none);
    }
    return PPR_OK;
  }
  // test knobs, read per call
  const int64_t wave_max = pprpairs::clamp_wave_max(env_i64("PPR_PR_WAVE_MAX", pprpairs::PR_WAVE_MAX_DEFAULT));
  const int64_t split = pprpairs::clamp_split(env_i64("PPR_PR_SPLIT", pprpairs::PR_SPLIT_DEFAULT));
  const int64_t chunk_groups = pprpairs::clamp_chunk(env_i64("PPR_PR_CHUNK", pprpairs::PR_CHUNK_DEFAULT));
  const bool binary = pprpairs::pr_use_binary(env_i64("PPR_PR_SEARCH", pprpairs::PR_SEARCH_AUTO), p->L);

  ResidentCall call;
  {
    const int rc = call.begin(p, iterations_run);
    if (rc) return rc;
  }
  const bool hk = p->hot_n > 0;
  {
    int Lp = WAVE;
    while (Lp < (int)p->L) Lp <<= 1;
    const size_t lds = pprk::p_lds((int)p->L, Lp, true);
    const int rc = hk ? set_pairs_lds<true>(lds) : set_pairs_lds<false>(lds);
    if (rc) return rc;
  }
  const bool rank_scratch = cls == pprpairs::PR_LOOKUP && (outs & pprpairs::PR_RANK);
  const std::vector<PChunk> chunks = pprpairs::cut_chunks(Q, gptr, chunk_groups, pprpairs::PR_CHUNK_PAIRS,
                                                          rank_scratch ? (int64_t)p->L : 0, pprpairs::PR_CHUNK_ENTRIES);
  pprpairs::PCount cnt;
  cnt.pairs = P;
  cnt.groups = Q;
  int64_t tiers[3] = {0, 0, 0};
  for (const PChunk& ck : chunks) {
    if (ck.j1 == ck.j0 && !(outs & pprpairs::PR_SLEN)) continue;  // groups without candidates only
    const int rc = hk ? pairs_chunk<true>(p, call, ck, gptr, sources, cands, outs, cls, out, wave_max, split, binary, cnt, tiers)
                      : pairs_chunk<false>(p, call, ck, gptr, sources, cands, outs, cls, out, wave_max, split, binary, cnt, tiers);
    if (rc) return rc;
  }
  if (st) {
    st->device_ms = call.dev_ms;
    st->pairs = P;
    st->groups = Q;
    st->lookup_pairs = cls == pprpairs::PR_LOOKUP ? P : 0;
    st->overlap_pairs = cls == pprpairs::PR_OVERLAP ? P : 0;
    st->entries_read = cnt.task_entries + cnt.cand_entries + cnt.slen_entries + cnt.clen_entries;
    st->algo_bytes = pprpairs::pr_algo_bytes(cls, outs, cnt);
    st->wave_groups = tiers[pprpairs::PR_TIER_WAVE];
    st->wg_groups = tiers[pprpairs::PR_TIER_WG];
    st->split_groups = tiers[pprpairs::PR_TIER_SPLIT];
    st->chunks = (int32_t)std::min<int64_t>((int64_t)chunks.size(), INT32_MAX);
  }
  return PPR_OK;
}

}  // namespace

extern "C" int ppr_grank_plan_pairs(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* gptr,
                                    const int32_t* sources, const int32_t* cands, uint32_t flags, double* out_fwd,
                                    double* out_bwd, uint8_t* out_hit, int32_t* out_rank, int32_t* out_common,
                                    double* out_dot, int32_t* out_slen, int32_t* out_clen, ppr_pairs_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- every refusal is decided here, on the host, before any kernel is launched
  const bool plan_ok = p && !p->mc && iterations_run >= 0;
  const uint32_t outs = (out_fwd ? pprpairs::PR_FWD : 0u) | (out_bwd ? pprpairs::PR_BWD : 0u) | (out_hit ? pprpairs::PR_HIT : 0u) |
                        (out_rank ? pprpairs::PR_RANK : 0u) | (out_common ? pprpairs::PR_COMMON : 0u) |
                        (out_dot ? pprpairs::PR_DOT : 0u) | (out_slen ? pprpairs::PR_SLEN : 0u) |
                        (out_clen ? pprpairs::PR_CLEN : 0u);
  {
    const int rc = pprpairs::check_pairs_args(plan_ok, Q, gptr, sources != nullptr, cands != nullptr, flags, outs);
    if (rc) return rc;
  }
  if (pprpairs::check_pairs_sizes(Q, gptr[Q])) return PPR_ERR_RANGE;
  if (pprpairs::check_ids(sources, Q, p->n) || pprpairs::check_ids(cands, gptr[Q], p->n)) return PPR_ERR_SOURCE;
  const PairsOut out{out_fwd, out_bwd, out_hit, out_rank, out_common, out_dot, out_slen, out_clen};
  return pairs_core(p, iterations_run, Q, gptr, sources, cands, outs, out, st);
}
