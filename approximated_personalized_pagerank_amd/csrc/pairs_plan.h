// pairs_plan.h -- host planning of the node-pair scores (ppr_grank_plan_pairs; pairs.hip) and the
// rules the host and the device share. Pure host code apart from the host/device rules:
// tests/cpp/pairs_plan_test.cpp includes only this header.
//
//   check_pairs_args   every refusal of a call that needs no id, in the order that is part of the contract
//   check_pairs_sizes  Q and P against the 32-bit positions of the kernels
//   check_ids          every source and candidate in [0, n)
//   pr_class           lookup or overlap, from the outputs requested
//   pr_tier            the tier of a group from its candidates
//   cut_chunks         the call's chunks: bounded groups and bounded pairs (a chunk may end inside a group)
//   cut_tasks          a chunk's tasks: the pieces of its groups, split groups in bounded runs of candidates
//   pr_out_bytes, pr_algo_bytes   the byte accounting of ppr_pairs_stats::algo_bytes
//   Limbs, pr_split, pr_add, pr_join   the 96-bit sums of the wave reduction as 32-bit limbs in 64-bit words
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ppr_hip.h"

#if defined(__HIPCC__)
#define PR_HD __host__ __device__
#else
#define PR_HD
#endif

namespace pprpairs {

// outputs requested, one bit each (the order of the C call's pointers)
enum : uint32_t {
  PR_FWD = 1, PR_BWD = 2, PR_HIT = 4, PR_RANK = 8, PR_COMMON = 16, PR_DOT = 32, PR_SLEN = 64, PR_CLEN = 128
};
constexpr int PR_LOOKUP = 0, PR_OVERLAP = 1;
constexpr int PR_TIER_WAVE = 0, PR_TIER_WG = 1, PR_TIER_SPLIT = 2;
constexpr uint32_t PR_FLAGS = 0u;  // no flag is defined
constexpr int64_t PR_MAX_COUNT = 0x7fffffff;  // most groups and most pairs of a call
// A wave streams one candidate row per trip, so a group of a few candidates is one wave's work and a
// workgroup's barriers and shared row only pay from about a wave's worth of trips per wave on; beyond
// 1024 candidates a group is cut so that a 4096-group call still gives every CU several tasks.
constexpr int64_t PR_WAVE_MAX_DEFAULT = 16, PR_SPLIT_DEFAULT = 1024;
// chunk: 2^15 groups, 2^21 pairs (at most 45 B each in scratch) and 2^22 rank entries (2 B each)
constexpr int64_t PR_CHUNK_DEFAULT = 1 << 15, PR_CHUNK_PAIRS = 1 << 21, PR_CHUNK_ENTRIES = 1 << 22;
constexpr int PR_SEARCH_AUTO = 0, PR_SEARCH_LINEAR = 1, PR_SEARCH_BINARY = 2;
constexpr int PR_BINARY_FROM_L = 512;  // auto: rows at least this wide (segments of 8 and more) are searched by bisection

// ---- refusals ----------------------------------------------------------------------------------
// The order of the checks is part of the contract: a call that is wrong in two ways gets the code of
// the first one below. `plan_ok`: a GRank plan (not null, not MC) and iterations_run >= 0. Reads
// gptr[0 .. Q] once Q >= 0 and gptr is there, and nothing else.
inline int check_pairs_args(bool plan_ok, int64_t Q, const int64_t* gptr, bool sources_given, bool cands_given,
                            uint32_t flags, uint32_t outs) {
  if (!plan_ok || !gptr || Q < 0) return PPR_ERR_ARG;
  if (gptr[0] != 0) return PPR_ERR_ARG;
  for (int64_t q = 0; q < Q; q++)
    if (gptr[q + 1] < gptr[q]) return PPR_ERR_ARG;
  if (Q > 0 && !sources_given) return PPR_ERR_ARG;
  if (gptr[Q] > 0 && !cands_given) return PPR_ERR_ARG;
  if (flags & ~PR_FLAGS) return PPR_ERR_ARG;
  if (outs == 0u) return PPR_ERR_ARG;
  return PPR_OK;
}
// positions are 32-bit in the kernels
inline int check_pairs_sizes(int64_t Q, int64_t P) { return (Q > PR_MAX_COUNT || P > PR_MAX_COUNT) ? PPR_ERR_RANGE : PPR_OK; }
// every id in [0, n), else PPR_ERR_SOURCE
inline int check_ids(const int32_t* ids, int64_t count, int64_t n) {
  for (int64_t i = 0; i < count; i++)
    if (ids[i] < 0 || (int64_t)ids[i] >= n) return PPR_ERR_SOURCE;
  return PPR_OK;
}

// ---- classes and tiers -------------------------------------------------------------------------
// the overlap of two rows needs a pass over both; everything else is a probe of one segment
PR_HD inline int pr_class(uint32_t outs) { return (outs & (PR_COMMON | PR_DOT)) ? PR_OVERLAP : PR_LOOKUP; }

// knob values as the call uses them
inline int64_t clamp_wave_max(int64_t v) { return std::max<int64_t>(0, std::min(v, PR_MAX_COUNT)); }
inline int64_t clamp_split(int64_t v) { return std::max<int64_t>(1, std::min(v, PR_CHUNK_PAIRS)); }
inline int64_t clamp_chunk(int64_t v) { return std::max<int64_t>(1, std::min(v, PR_MAX_COUNT)); }

// split: more than `split` candidates; wave: at most wave_max (0 closes the tier); else one workgroup.
// Every group gets exactly one tier; a group without candidates gets one too and no task.
PR_HD inline int pr_tier(int64_t ncand, int64_t wave_max, int64_t split) {
  if (ncand > split) return PR_TIER_SPLIT;
  if (wave_max > 0 && ncand <= wave_max) return PR_TIER_WAVE;
  return PR_TIER_WG;
}

// bisection or a linear scan of the LDS segment (knob PPR_PR_SEARCH)
inline bool pr_use_binary(int64_t knob, int64_t L) {
  if (knob == PR_SEARCH_LINEAR) return false;
  if (knob == PR_SEARCH_BINARY) return true;
  return L >= PR_BINARY_FROM_L;
}

// ---- chunks ------------------------------------------------------------------------------------
// One chunk: the pairs [j0, j1) and the groups [q0, q1) that hold them (the first and the last group
// may continue in a neighbouring chunk: a position's result is fixed by j alone and every sum is
// exact, so a group cut anywhere gives the same bits). At most `chunk_groups` groups -- by the row
// budget of the rank scratch at most max(1, entry_budget / width) when `width` > 0 -- and at most
// `pair_budget` pairs. The chunks cover [0, Q) and [0, P) in order; groups without candidates belong
// to exactly one chunk.
struct PChunk {
  int64_t q0, q1, j0, j1;
};
inline std::vector<PChunk> cut_chunks(int64_t Q, const int64_t* gptr, int64_t chunk_groups, int64_t pair_budget,
                                      int64_t width, int64_t entry_budget) {
  std::vector<PChunk> out;
  chunk_groups = std::max<int64_t>(1, chunk_groups);
  pair_budget = std::max<int64_t>(1, pair_budget);
  if (width > 0) chunk_groups = std::min(chunk_groups, std::max<int64_t>(1, entry_budget / width));
  int64_t q = 0, j = 0;  // next group, next pair (gptr[q] <= j <= gptr[q + 1] when q < Q)
  while (q < Q) {
    PChunk c{q, q, j, j};
    while (c.q1 < Q && c.q1 - c.q0 < chunk_groups) {
      const int64_t e = gptr[c.q1 + 1];
      const int64_t room = pair_budget - (c.j1 - c.j0);
      if (e - c.j1 <= room) {  // the rest of the group fits
        c.j1 = e;
        c.q1++;
        continue;
      }
      if (c.j1 > c.j0 && c.j1 == gptr[c.q1]) break;  // a group that does not fit starts the next chunk
      c.j1 += room;                                   // ... unless it is more than a chunk: a piece of it
      break;
    }
    // the group the chunk ends in, when it continues
    int64_t qe = c.q1;
    if (qe < Q && c.j1 > gptr[qe]) qe++;
    out.push_back(PChunk{c.q0, qe, c.j0, c.j1});
    j = c.j1;
    q = c.q1;
  }
  return out;
}

// ---- tasks -------------------------------------------------------------------------------------
struct PTask {        // one wave or one workgroup: candidates [j0, j1) of the chunk, all of group g
  int32_t g;          // group (chunk index)
  int32_t j0, j1;     // chunk positions
  int32_t pad;
};
// The tasks of chunk c. A group's tier comes from all its candidates (not from the piece in this
// chunk); its piece goes to the wave list whole, to the workgroup list whole, or -- split -- to the
// workgroup list in runs of `split` candidates. A piece without candidates gets no task. The tier
// counters count a group in the chunk it starts in.
inline void cut_tasks(const PChunk& c, const int64_t* gptr, int64_t wave_max, int64_t split, std::vector<PTask>& wave,
                      std::vector<PTask>& wg, int64_t tiers[3]) {
  wave.clear();
  wg.clear();
  split = std::max<int64_t>(1, split);
  for (int64_t q = c.q0; q < c.q1; q++) {
    const int64_t b = gptr[q], e = gptr[q + 1];
    const int t = pr_tier(e - b, wave_max, split);
    // a group starts in the chunk whose pair range holds its first position (a group without
    // candidates: in the chunk whose group range holds it; cut_chunks gives it to exactly one)
    if (b < e ? (b >= c.j0 && b < c.j1) : true) tiers[t]++;
    const int64_t a0 = std::max(b, c.j0), a1 = std::min(e, c.j1);
    if (a1 <= a0) continue;
    const int32_t g = (int32_t)(q - c.q0);
    if (t == PR_TIER_WAVE) {
      wave.push_back(PTask{g, (int32_t)(a0 - c.j0), (int32_t)(a1 - c.j0), 0});
    } else if (t == PR_TIER_WG) {
      wg.push_back(PTask{g, (int32_t)(a0 - c.j0), (int32_t)(a1 - c.j0), 0});
    } else {
      for (int64_t j = a0; j < a1; j += split)
        wg.push_back(PTask{g, (int32_t)(j - c.j0), (int32_t)(std::min(a1, j + split) - c.j0), 0});
    }
  }
}

// ---- byte accounting ---------------------------------------------------------------------------
// bytes written per pair / per group for the outputs requested
PR_HD inline int64_t pr_pair_out_bytes(uint32_t outs) {
  return ((outs & PR_FWD) ? 8 : 0) + ((outs & PR_BWD) ? 8 : 0) + ((outs & PR_HIT) ? 1 : 0) + ((outs & PR_RANK) ? 4 : 0) +
         ((outs & PR_COMMON) ? 4 : 0) + ((outs & PR_DOT) ? 8 : 0) + ((outs & PR_CLEN) ? 4 : 0);
}
PR_HD inline int64_t pr_group_out_bytes(uint32_t outs) { return (outs & PR_SLEN) ? 4 : 0; }

// What a call counted (the kernels' counters and the host's): see ppr_pairs_stats::algo_bytes in
// include/ppr_hip.h, which this restates term by term.
struct PCount {
  int64_t pairs = 0, groups = 0;
  int64_t tasks = 0;         // overlap: group tasks
  int64_t ranked_groups = 0; // lookup with rank: rows k_p_rank built
  int64_t task_entries = 0;  // overlap: sum over the tasks of len(u); lookup with rank: sum over the groups of len(u)
  int64_t cand_entries = 0;  // overlap: sum over the pairs of len(v); lookup: ids of the probed segments
  int64_t hits = 0;          // overlap: sum of common; lookup: forward and backward hits
  int64_t fwd_hits = 0;      // lookup with rank: forward hits (each reads its rank)
  int64_t slen_entries = 0;  // with out_slen: sum over the groups of len(u)
  int64_t clen_entries = 0;  // lookup with out_clen: sum over the pairs of len(v)
};
inline int64_t pr_algo_bytes(int cls, uint32_t outs, const PCount& c) {
  int64_t b = c.pairs * (pr_pair_out_bytes(outs) + 4) + c.groups * (pr_group_out_bytes(outs) + 4) + 4 * c.slen_entries;
  if (cls == PR_OVERLAP) {
    b += 12 * c.task_entries + 128 * c.tasks + ((outs & PR_RANK) ? 2 * c.task_entries : 0);
    b += 4 * c.cand_entries + ((outs & PR_DOT) ? 8 * c.hits : 0);
  } else {
    b += c.pairs * (8 + 4) + 4 * c.cand_entries + 8 * c.hits + 4 * c.clen_entries;
    if (outs & PR_RANK) b += 14 * c.task_entries + 128 * c.ranked_groups + 2 * c.fwd_hits;
  }
  return b;
}

// ---- the 96-bit sums of the wave reduction -----------------------------------------------------
// A value X < 2^96 as three 32-bit limbs, each in a 64-bit word: limb sums are plain 64-bit adds
// without carries -- up to 2^32 values can be added before a word could overflow -- in any order and
// any grouping (the lanes of a wave by butterflies, a lane's hits one after the other), and the
// carries are propagated once, when the words are joined. The CPU test runs these very functions.
struct Limbs {
  unsigned long long w0, w1, w2;
};
PR_HD inline Limbs pr_split(unsigned long long lo, uint32_t hi) {
  return Limbs{lo & 0xffffffffull, lo >> 32, (unsigned long long)hi};
}
PR_HD inline Limbs pr_add(const Limbs& a, const Limbs& b) { return Limbs{a.w0 + b.w0, a.w1 + b.w1, a.w2 + b.w2}; }
// X mod 2^96 of the limb sums: lo = bits 0..63, hi = bits 64..95
PR_HD inline void pr_join(const Limbs& s, unsigned long long& lo, uint32_t& hi) {
  const unsigned long long t1 = s.w1 + (s.w0 >> 32);
  const unsigned long long t2 = s.w2 + (t1 >> 32);
  lo = (s.w0 & 0xffffffffull) | (t1 << 32);
  hi = (uint32_t)t2;
}

}  // namespace pprpairs
