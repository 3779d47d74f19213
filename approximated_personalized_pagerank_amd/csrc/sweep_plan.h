// sweep_plan.h -- host planning of the sweep-cut local clustering (ppr_grank_plan_sweep,
// ppr_grank_plan_sweep_vectors; sweep.hip) and the rules the host and the device share. Pure host
// code apart from the host/device rules: tests/cpp/sweep_plan_test.cpp includes only this header.
//
//   check_sweep_args   every refusal of a call, in the order that is part of the contract
//   check_vectors      the refusals of caller-supplied rows (lengths, scores, ids)
//   sw_tier            the tier of a source from its walk size W (edges) and its members
//   sw_table_slots     slots of the key -> rank table of a source
//   cut_slices         the (source, edge slice) tasks of the slice tier, in batches of bounded rows
//   cut_chunks         the call's chunks: bounded sources and bounded row entries
//   frac_less          cut_a / den_a < cut_b / den_b, exactly (128-bit products)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ppr_hip.h"

#if defined(__HIPCC__)
#define SW_HD __host__ __device__
#else
#define SW_HD
#endif

namespace pprsweep {

constexpr int SW_MAX_WIDTH = 4096;       // widest row (max_size, width_in)
constexpr int SW_WAVE_T = 256;           // table of the wave tier
constexpr int SW_MIN_T = 256, SW_MAX_T = 8192;
// planner verdict of one source: wave | SW_CODE_WG + log2 T | slice
constexpr int SW_CODE_WAVE = 0, SW_CODE_WG = 0x100, SW_CODE_SLICE = 0x200;
constexpr int64_t SW_WAVE_MAX_DEFAULT = 2048, SW_WG_MAX_DEFAULT = 1 << 17, SW_SLICE_DEFAULT = 1 << 15;
constexpr int64_t SW_EDGE_LIMIT = (int64_t)1 << 30;  // a workgroup's share of edges: 32-bit LDS bins, int numbering
constexpr int64_t SW_CHUNK_DEFAULT = 1 << 15, SW_CHUNK_ENTRIES = 1 << 22, SW_BATCH_ENTRIES = 1 << 22;

// the smallest power-of-two table (>= SW_MIN_T) that `members` keys fill to at most 3/4
SW_HD inline int sw_table_slots(int members) {
  int T = SW_MIN_T;
  while (T < SW_MAX_T && 4 * (int64_t)members > 3 * (int64_t)T) T <<= 1;
  return T;
}
SW_HD inline int sw_log2(int T) {
  int lg = 0;
  while ((1 << lg) < T) lg++;
  return lg;
}

// wave: W <= wave_max and the members fit the wave tier's table; workgroup: W <= wg_max; else slices.
// wave_max / wg_max = 0 close a tier (the knobs of the tests); every source gets exactly one tier.
SW_HD inline int sw_tier(int64_t W, int members, int64_t wave_max, int64_t wg_max) {
  if (wave_max > 0 && W <= wave_max && 4 * members <= 3 * SW_WAVE_T) return SW_CODE_WAVE;
  if (wg_max > 0 && W <= wg_max) return SW_CODE_WG + sw_log2(sw_table_slots(members));
  return SW_CODE_SLICE;
}

// knob values as the call uses them
inline int64_t clamp_wave_max(int64_t v) { return std::max<int64_t>(0, std::min(v, SW_EDGE_LIMIT)); }
inline int64_t clamp_wg_max(int64_t v) { return std::max<int64_t>(0, std::min(v, SW_EDGE_LIMIT)); }
inline int64_t clamp_slice(int64_t v) { return std::max<int64_t>(64, std::min(v, SW_EDGE_LIMIT)); }

// ---- exact comparison of two ratios ------------------------------------------------------------
struct U128 {
  uint64_t hi, lo;
};
SW_HD inline U128 mul64(uint64_t a, uint64_t b) {
  const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);
  U128 r;
  r.lo = (p00 & 0xffffffffu) | (mid << 32);
  r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  return r;
}
// cut_a / den_a < cut_b / den_b for nonnegative cuts and positive denominators: cut_a den_b < cut_b den_a
SW_HD inline bool frac_less(int64_t cut_a, int64_t den_a, int64_t cut_b, int64_t den_b) {
  const U128 x = mul64((uint64_t)cut_a, (uint64_t)den_b), y = mul64((uint64_t)cut_b, (uint64_t)den_a);
  return x.hi != y.hi ? x.hi < y.hi : x.lo < y.lo;
}

// ---- refusals ----------------------------------------------------------------------------------
// width of a result row: max_size, or the row width when max_size is 0 (vectors: never above width_in)
inline int64_t sweep_width(uint32_t max_size, int64_t row_width, bool vectors) {
  if (max_size == 0) return row_width;
  return vectors ? std::min<int64_t>(max_size, row_width) : (int64_t)max_size;
}

// The order of the checks is part of the contract: a call that is wrong in two ways gets the code of
// the first one below. `plan_ok`: a GRank plan (not null, not MC) and, for the resident rows,
// iterations_run >= 0. rows = S (sources) or R (vectors); `ids_given`: the sources pointer, or the
// three row pointers of a vectors call. row_width = L or width_in.
inline int check_sweep_args(bool plan_ok, int64_t n, int64_t m, int64_t rows, bool ids_given, bool vectors,
                            int64_t row_width, uint32_t min_size, uint32_t max_size, int64_t max_vol, uint32_t flags,
                            bool outs_ok, bool prof_cut, bool prof_vol) {
  if (!plan_ok || rows < 0) return PPR_ERR_ARG;
  if (vectors ? (!ids_given && rows > 0) : (!ids_given && rows != n)) return PPR_ERR_ARG;
  if (flags != 0u) return PPR_ERR_ARG;
  if (prof_cut != prof_vol) return PPR_ERR_ARG;
  if (rows > 0 && !outs_ok) return PPR_ERR_ARG;
  if (row_width < 0) return PPR_ERR_ARG;
  if (max_size > (uint32_t)SW_MAX_WIDTH || row_width > SW_MAX_WIDTH) return PPR_ERR_RANGE;
  const int64_t width = sweep_width(max_size, row_width, vectors);
  if (min_size == 0u || (int64_t)min_size > width) return PPR_ERR_ARG;
  if (max_vol < 0 || max_vol > m) return PPR_ERR_ARG;
  return PPR_OK;
}

// every id in [0, n), else PPR_ERR_SOURCE
inline int check_sources(const int32_t* ids, int64_t count, int64_t n) {
  for (int64_t i = 0; i < count; i++)
    if (ids[i] < 0 || (int64_t)ids[i] >= n) return PPR_ERR_SOURCE;
  return PPR_OK;
}

// R rows of width_in: a length outside [0, width_in], a negative / NaN / infinite score or a repeated
// id within a row is PPR_ERR_ARG, an id outside [0, n) PPR_ERR_SOURCE; the first row that is wrong
// decides, and within it lengths go before scores, scores before id ranges, ranges before repeats.
inline int check_vectors(int64_t R, int64_t width_in, const int32_t* ids, const double* scores, const int32_t* lens,
                         int64_t n) {
  std::vector<int32_t> tmp;
  for (int64_t r = 0; r < R; r++) {
    const int64_t len = lens[r];
    if (len < 0 || len > width_in) return PPR_ERR_ARG;
    const int32_t* k = ids + r * width_in;
    const double* s = scores + r * width_in;
    for (int64_t i = 0; i < len; i++)
      if (!(s[i] >= 0.0) || !std::isfinite(s[i])) return PPR_ERR_ARG;
    if (check_sources(k, len, n)) return PPR_ERR_SOURCE;
    tmp.assign(k, k + len);
    std::sort(tmp.begin(), tmp.end());
    if (std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end()) return PPR_ERR_ARG;
  }
  return PPR_OK;
}

// ---- chunks ------------------------------------------------------------------------------------
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

// ---- the slice tier ----------------------------------------------------------------------------
struct STask {        // one k_s_slice workgroup: edges [e0, e1) of the source's walk
  int64_t e0, e1;
  int32_t q;          // source (chunk index)
  int32_t row;        // its row of the batch's global histogram
};
struct SBatch {
  int64_t t0, t1;     // tasks
  int64_t r0, r1;     // entries of `list`
};
// list[i]: chunk index of the i-th slice-tier source, W[i] its walk size. Slices of `slice` edges
// cover [0, W) once, in order (W = 0: one empty slice, so that every source has a task); a batch
// holds at most max(1, row_budget) histogram rows.
inline void cut_slices(const int32_t* list, const int64_t* W, int64_t count, int64_t slice, int64_t row_budget,
                       std::vector<STask>& tasks, std::vector<SBatch>& batches) {
  tasks.clear();
  batches.clear();
  if (slice < 1) slice = 1;
  if (row_budget < 1) row_budget = 1;
  for (int64_t i = 0; i < count;) {
    SBatch b{(int64_t)tasks.size(), 0, i, i};
    while (b.r1 < count && b.r1 - b.r0 < row_budget) {
      const int64_t w = W[b.r1] < 0 ? 0 : W[b.r1];
      int64_t e0 = 0;
      do {
        const int64_t e1 = w - e0 < slice ? w : e0 + slice;
        tasks.push_back(STask{e0, e1, list[b.r1], (int32_t)(b.r1 - b.r0)});
        e0 = e1;
      } while (e0 < w);
      b.r1++;
    }
    b.t1 = (int64_t)tasks.size();
    batches.push_back(b);
    i = b.r1;
  }
}

}  // namespace pprsweep
