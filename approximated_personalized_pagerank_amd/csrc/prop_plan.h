// prop_plan.h -- host planning of the transposed feature propagation (ppr_grank_plan_propagate_t,
// propagate.hip) and the weight rule both directions share. Pure host code apart from the
// host/device weight rule: tests/cpp/prop_plan_test.cpp includes only this header.
//
//   cut_key_ranges     the passes: consecutive key ranges whose postings sum to at most E (a key
//                      with more than E postings gets a range to itself), from the per-key counts.
//                      A key's whole list lives in one pass, so no result depends on E.
//   build_chunk_tasks  one pass's tasks from the run starts of its sorted postings: a key's list is
//                      cut into chunks of PROP_CHUNK postings; a key with one chunk writes its
//                      output row directly (part = -1), a key with more writes one fp64 partial
//                      row per chunk (consecutive slots, in chunk order) and gets a fold task.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PROP_HD __host__ __device__
#else
#define PROP_HD
#endif

namespace pprprop {

constexpr int PROP_CHUNK = 512;  // PPR_PROP_CHUNK (include/ppr_hip.h): part of the contract

// weight of an entry with score s in a row whose scores sum to W (PPR_PROP_ROW_NORMALIZE)
PROP_HD inline double prop_weight(double s, double W) { return W == 0.0 ? 0.0 : s / W; }
// W = ((0.0 + s_0) + s_1) + ... in stored order
inline double prop_row_sum(const double* s, int len) {
  double W = 0.0;
  for (int j = 0; j < len; j++) W = W + s[j];
  return W;
}

struct KeyRange {
  int64_t k0, k1;     // keys [k0, k1)
  int64_t postings;
};

// Every key of [0, n) lies in exactly one range (keys without postings too: the pass that owns them
// zeroes their output rows); n = 0 gives no range.
inline std::vector<KeyRange> cut_key_ranges(const int32_t* cnt, int64_t n, int64_t E) {
  std::vector<KeyRange> out;
  if (E < 1) E = 1;
  int64_t k0 = 0, sum = 0;
  for (int64_t k = 0; k < n; k++) {
    const int64_t c = cnt[k] < 0 ? 0 : cnt[k];
    if (k > k0 && sum + c > E) {
      out.push_back(KeyRange{k0, k, sum});
      k0 = k;
      sum = 0;
    }
    sum += c;
  }
  if (n > 0) out.push_back(KeyRange{k0, n, sum});
  return out;
}

struct PTask {        // one k_p_tsum wave per (task, column tile)
  int64_t off;        // first posting of the chunk in the pass's sorted arrays
  int64_t part;       // partial row it writes, -1: the key's only chunk, writes the output row
  int32_t key;        // dense id (not relative to the range)
  int32_t n;          // postings, 1 .. PROP_CHUNK
};
struct PFold {        // one k_p_tfold block: output row = ((p_0 + p_1) + p_2) ... in chunk order
  int64_t part;       // first of its m consecutive partial rows
  int32_t key;
  int32_t m;
};
struct ChunkPlan {
  std::vector<PTask> tasks;
  std::vector<PFold> folds;
  int64_t nparts = 0;
  int64_t nzero = 0;  // keys of the range without postings
};

// start[0 .. nk]: start[k] = first sorted posting of key k0 + k, start[nk] = postings of the pass
// (non-decreasing; a decreasing pair is read as an empty list)
inline void build_chunk_tasks(const int32_t* start, int64_t nk, int64_t k0, int chunk, ChunkPlan& out) {
  out.tasks.clear();
  out.folds.clear();
  out.nparts = 0;
  out.nzero = 0;
  if (chunk < 1) chunk = 1;
  for (int64_t k = 0; k < nk; k++) {
    const int64_t b = start[k], e = start[k + 1];
    if (e <= b) { out.nzero++; continue; }
    const int64_t m = (e - b + chunk - 1) / chunk;
    if (m > 1) out.folds.push_back(PFold{out.nparts, (int32_t)(k0 + k), (int32_t)m});
    for (int64_t c = 0; c < m; c++) {
      const int64_t o = b + c * chunk;
      const int64_t len = e - o < chunk ? e - o : chunk;
      out.tasks.push_back(PTask{o, m > 1 ? out.nparts++ : -1, (int32_t)(k0 + k), (int32_t)len});
    }
  }
}

// Columns per block of the transposed sum: the partial rows of a block (nparts x cols fp64) stay
// within `budget` bytes; a multiple of `tile` columns, at least one tile, at most F rounded up.
inline int prop_col_block(int64_t nparts, int F, int tile, int64_t budget) {
  const int full = (F + tile - 1) / tile * tile;
  if (nparts <= 0) return full;
  int64_t cols = budget / (8 * nparts) / tile * tile;
  if (cols < tile) cols = tile;
  return cols > full ? full : (int)cols;
}

}  // namespace pprprop
