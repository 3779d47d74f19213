// subgraph_plan.h -- host planning of the PPR-induced subgraph batches (ppr_grank_plan_subgraphs;
// subgraph.hip) and the rules the host and the device share. Pure host code apart from the
// host/device rules: tests/cpp/subgraph_plan_test.cpp includes only this header.
//
//   check_subg_args    every refusal of a call, in the order that is part of the contract
//   sg_width           members kept per source at most
//   sg_eff_deg         a member's out-edges as the walk counts them (0 when max_deg caps it)
//   sg_tier            the tier of a source from its walk size W (edges) and its members
//   sg_table_slots     slots of the key -> rank table of a source
//   sg_groups          the 64-edge groups of a source's walk: the numbering both passes share
//   cut_chunks         the call's chunks: bounded sources and bounded row entries
//   cut_batches        a chunk's walk batches: bounded members and bounded groups
//   cut_slices         the (source, group range) tasks of the slice tier
//   sg_capacity        the capacity and index-type verdict of a finished count
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ppr_hip.h"

#if defined(__HIPCC__)
#define SG_HD __host__ __device__
#else
#define SG_HD
#endif

namespace pprsubg {

constexpr int SG_MAX_WIDTH = 4096;       // most members of one source (size)
constexpr int SG_WAVE_T = 256;           // table of the wave tier
constexpr int SG_MIN_T = 256, SG_MAX_T = 8192;
constexpr int SG_GROUP = 64;             // edges per group = lanes of a wave
// planner verdict of one source: wave | SG_CODE_WG + log2 T | slice
constexpr int SG_CODE_WAVE = 0, SG_CODE_WG = 0x100, SG_CODE_SLICE = 0x200;
// The walk is the sweep's (one coalesced read of the adjacency word and one LDS probe per edge), so
// the tier thresholds are the sweep's: below ~2 K edges a workgroup's barriers and table fill cost
// more than the walk; beyond 2^17 edges one workgroup is a tail, and 2^15-edge slices keep >= 4 of them.
constexpr int64_t SG_WAVE_MAX_DEFAULT = 2048, SG_WG_MAX_DEFAULT = 1 << 17, SG_SLICE_DEFAULT = 1 << 15;
constexpr int64_t SG_EDGE_LIMIT = (int64_t)1 << 30;  // most walked edges of one source: int numbering, 32-bit counters
constexpr int64_t SG_MAX_SOURCES = (int64_t)1 << 30;
// chunk: 2^15 sources and 2^21 row entries (12 B each in scratch); walk batch: 2^22 groups (2^28 edges;
// two 4-byte words per group) and 2^21 members (two 8-byte words each)
constexpr int64_t SG_CHUNK_DEFAULT = 1 << 15, SG_CHUNK_ENTRIES = 1 << 21;
constexpr int64_t SG_BATCH_GROUPS = 1 << 22, SG_BATCH_MEMBERS = 1 << 21;
constexpr uint32_t SG_FLAGS = (uint32_t)(PPR_SUBG_ROOT_FIRST | PPR_SUBG_IDX64);

// the smallest power-of-two table (>= SG_MIN_T) that `members` keys fill to at most 3/4
SG_HD inline int sg_table_slots(int members) {
  int T = SG_MIN_T;
  while (T < SG_MAX_T && 4 * (int64_t)members > 3 * (int64_t)T) T <<= 1;
  return T;
}
SG_HD inline int sg_log2(int T) {
  int lg = 0;
  while ((1 << lg) < T) lg++;
  return lg;
}

// wave: W <= wave_max and the members fit the wave tier's table; workgroup: W <= wg_max; else slices.
// wave_max / wg_max = 0 close a tier (the knobs of the tests); every source gets exactly one tier.
SG_HD inline int sg_tier(int64_t W, int members, int64_t wave_max, int64_t wg_max) {
  if (wave_max > 0 && W <= wave_max && 4 * members <= 3 * SG_WAVE_T) return SG_CODE_WAVE;
  if (wg_max > 0 && W <= wg_max) return SG_CODE_WG + sg_log2(sg_table_slots(members));
  return SG_CODE_SLICE;
}

// A member's out-edges as the walk counts them: 0 when max_deg (> 0) caps it, else its degree clamped
// to [0, SG_EDGE_LIMIT + 1], so that the sum over 4096 members cannot overflow and a source beyond
// the limit is still seen to be beyond it.
SG_HD inline int64_t sg_eff_deg(int64_t deg, int64_t max_deg) {
  if (deg < 0) deg = 0;
  if (max_deg > 0 && deg > max_deg) return 0;
  return deg > SG_EDGE_LIMIT ? SG_EDGE_LIMIT + 1 : deg;
}

// The numbering of a source's walk. The members are taken in windows of 64 ranks; a window's edges
// (its members' adjacency lists one behind the other) are cut into groups of 64, the last one of a
// window may be short; the groups of the windows are numbered one behind the other. Both passes and
// every tier use this numbering, and a slice is a range of it.
SG_HD inline int64_t sg_window_groups(int64_t window_edges) { return (window_edges + SG_GROUP - 1) / SG_GROUP; }
inline int64_t sg_groups(const int64_t* eff_deg, int members) {
  int64_t g = 0;
  for (int w0 = 0; w0 < members; w0 += SG_GROUP) {
    int64_t t = 0;
    for (int i = w0; i < members && i < w0 + SG_GROUP; i++) t += eff_deg[i];
    g += sg_window_groups(t);
  }
  return g;
}

// knob values as the call uses them
inline int64_t clamp_wave_max(int64_t v) { return std::max<int64_t>(0, std::min(v, SG_EDGE_LIMIT)); }
inline int64_t clamp_wg_max(int64_t v) { return std::max<int64_t>(0, std::min(v, SG_EDGE_LIMIT)); }
// groups per slice task from the knob in edges (at least one group)
inline int64_t slice_groups(int64_t slice_edges) {
  return std::max<int64_t>(1, std::min(slice_edges, SG_EDGE_LIMIT) / SG_GROUP);
}

// ---- refusals ----------------------------------------------------------------------------------
inline int64_t sg_width(uint32_t size, int64_t L) { return size == 0 ? L : (int64_t)size; }

// The order of the checks is part of the contract: a call that is wrong in two ways gets the code of
// the first one below. `plan_ok`: a GRank plan (not null, not MC) and iterations_run >= 0;
// `host_ptrs`: node_ptr and edge_ptr; nodes / rowptr / col are the required device pointers, scores /
// row / eid the optional ones. A count-only call has every device pointer null and both capacities 0.
inline int check_subg_args(bool plan_ok, int64_t n, int64_t S, bool sources_given, bool host_ptrs, uint32_t size,
                           int64_t max_deg, uint32_t flags, int64_t node_cap, int64_t edge_cap, bool nodes, bool rowptr,
                           bool col, bool scores, bool row, bool eid) {
  if (!plan_ok || !host_ptrs || S < 0) return PPR_ERR_ARG;
  if (!sources_given && S != n) return PPR_ERR_ARG;
  if (flags & ~SG_FLAGS) return PPR_ERR_ARG;
  if (max_deg < 0 || node_cap < 0 || edge_cap < 0) return PPR_ERR_ARG;
  const int req = (int)nodes + (int)rowptr + (int)col;
  if (req != 0 && req != 3) return PPR_ERR_ARG;
  if (req == 0 && (scores || row || eid || node_cap != 0 || edge_cap != 0)) return PPR_ERR_ARG;
  if (size > (uint32_t)SG_MAX_WIDTH || S > SG_MAX_SOURCES) return PPR_ERR_RANGE;
  return PPR_OK;
}

// every id in [0, n), else PPR_ERR_SOURCE
inline int check_sources(const int32_t* ids, int64_t count, int64_t n) {
  for (int64_t i = 0; i < count; i++)
    if (ids[i] < 0 || (int64_t)ids[i] >= n) return PPR_ERR_SOURCE;
  return PPR_OK;
}

// ---- capacities --------------------------------------------------------------------------------
// most elements the index type can number (the largest batch id is N - 1, the largest rowptr value E)
inline int64_t sg_index_limit(bool idx64) { return idx64 ? INT64_MAX : (int64_t)INT32_MAX; }
// may the edges [0, E) be written? (asked per batch with the running E: once false, no emit pass runs)
inline bool sg_edges_fit(int64_t E, int64_t edge_cap, bool idx64) { return E <= edge_cap && E <= sg_index_limit(idx64); }
// the verdict of a finished count: N nodes and E edges against the capacities and the index type
inline int sg_capacity(int64_t N, int64_t E, int64_t node_cap, int64_t edge_cap, bool idx64, bool count_only) {
  if (N > sg_index_limit(idx64) || E > sg_index_limit(idx64)) return PPR_ERR_RANGE;
  if (count_only) return PPR_OK;
  if (N > node_cap || E > edge_cap) return PPR_ERR_RANGE;
  return PPR_OK;
}

// ---- chunks and batches ------------------------------------------------------------------------
// boundaries b[0] = 0 < ... < b.back() = rows: a chunk holds at most `chunk_rows` rows and at most
// `budget` row entries (rows * width; a single row wider than the budget is a chunk of its own)
inline std::vector<int64_t> cut_chunks(int64_t rows, int64_t width, int64_t chunk_rows, int64_t budget) {
  std::vector<int64_t> b{0};
  if (chunk_rows < 1) chunk_rows = 1;
  const int64_t by_budget = std::max<int64_t>(1, budget / std::max<int64_t>(width, 1));
  const int64_t step = std::min(chunk_rows, by_budget);
  for (int64_t q = 0; q < rows; q += step) b.push_back(std::min(rows, q + step));
  return b;
}

// A chunk's sources in walk batches, boundaries as above: a batch holds at most `group_budget` groups
// and `member_budget` members (a single source beyond a budget is a batch of its own), so that the
// per-group and per-member scratch stays bounded whatever the sources walk.
inline std::vector<int64_t> cut_batches(const int64_t* groups, const int32_t* members, int64_t count, int64_t group_budget,
                                        int64_t member_budget) {
  std::vector<int64_t> b{0};
  int64_t g = 0, m = 0;
  for (int64_t i = 0; i < count; i++) {
    const int64_t gi = groups[i] < 0 ? 0 : groups[i], mi = members[i] < 0 ? 0 : members[i];
    if (i > b.back() && (g + gi > group_budget || m + mi > member_budget)) {
      b.push_back(i);
      g = m = 0;
    }
    g += gi;
    m += mi;
  }
  if (count > 0) b.push_back(count);
  return b;
}

// ---- the slice tier ----------------------------------------------------------------------------
struct GTask {        // one slice workgroup: groups [g0, g1) of the source's numbering
  int64_t g0, g1;
  int32_t q;          // source (chunk index)
  int32_t pad;
};
// list[i]: chunk index of the i-th slice-tier source, groups[i] its group count. Tasks of
// `per_task` groups cover [0, groups) once, in order; a source without groups gets no task.
inline void cut_slices(const int32_t* list, const int64_t* groups, int64_t count, int64_t per_task,
                       std::vector<GTask>& tasks) {
  tasks.clear();
  if (per_task < 1) per_task = 1;
  for (int64_t i = 0; i < count; i++) {
    const int64_t G = groups[i];
    for (int64_t g0 = 0; g0 < G; g0 += per_task) tasks.push_back(GTask{g0, G - g0 < per_task ? G : g0 + per_task, list[i], 0});
  }
}

}  // namespace pprsubg
