// sv_plan.h -- host planning rules of the sieve's device retries. Pure host code,
// no HIP: tests/cpp/sv_retry_grid_test.cpp compiles it alone.
//
// A retry launch (k_sv1_list behind a one-slice class, or the second k_svA -> k_svB -> k_svF chain of
// the multi-slice sources) costs CU time even where nothing overflowed: a 16-wave, 113-KB block that
// reads a zero and leaves still passes through a CU. So its grid comes from what the partition's
// last sieved updates of this job overflowed, not from a fixed share of the class.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace pprk {

// PPR_SV_RETRY_GRID: auto (the rule below), legacy (cnt / 8 + 64, retry chain always queued), full
// (the whole class), or an integer N >= 0 (N blocks: tests)
constexpr int SV_GRID_AUTO = -1, SV_GRID_LEGACY = -2, SV_GRID_FULL = -3;

inline int sv_retry_mode_parse(const char* s) {
  if (!s || !*s || !std::strcmp(s, "auto")) return SV_GRID_AUTO;
  if (!std::strcmp(s, "legacy")) return SV_GRID_LEGACY;
  if (!std::strcmp(s, "full")) return SV_GRID_FULL;
  char* end = nullptr;
  const long long v = std::strtoll(s, &end, 10);
  if (end == s || *end || v < 0) return SV_GRID_AUTO;
  return (int)std::min<long long>(v, 1 << 30);
}

// blocks of the retry launch behind a class of `cnt` sources (0: no retry launch). `seen`: sieved
// updates of this partition so far in this job in which the list had sources; `prev1`, `prev2`: the
// list's first overflows in the last such update and the one before (prev2 is only looked at from
// the third update on: a second update has observed one count, not two).
//   first update       the whole class (nothing is known; the early updates overflow the most)
//   later              2 prev1 + 64, at most the class
//   two updates with no overflow: no launch -- the class's overflows then go straight to the host
//   hand-back, unseeded (they are counted, so a later update retries again)
inline int64_t sv_retry_grid(int64_t cnt, int seen, int64_t prev1, int64_t prev2, int mode) {
  if (cnt <= 0) return 0;
  if (mode >= 0) return std::min<int64_t>(cnt, mode);
  if (mode == SV_GRID_FULL) return cnt;
  if (mode == SV_GRID_LEGACY) return std::min<int64_t>(cnt, cnt / 8 + 64);
  if (seen <= 0) return cnt;
  if (seen >= 2 && prev1 <= 0 && prev2 <= 0) return 0;
  return std::min<int64_t>(cnt, 2 * std::max<int64_t>(0, prev1) + 64);
}

// The last update's first overflows carried over to a class of another size. At a partition's early
// updates the class grows as rows fill up (a source enters the sieve with its first full row), and
// the new sources overflow like the old ones: the count is scaled by the growth, so the grid follows
// the overflow rate. A class that shrank keeps the count (the grid's margin covers it).
inline int64_t sv_scale_prev(int64_t prev1, int64_t prev_cnt, int64_t cnt) {
  if (prev1 <= 0 || prev_cnt <= 0 || cnt <= prev_cnt) return std::max<int64_t>(0, prev1);
  const double x = std::ceil((double)prev1 * ((double)cnt / (double)prev_cnt));
  return x >= (double)cnt ? cnt : (int64_t)x;
}

// per-partition overflow history of one job (ppr_plan::sv_hist; reset by every init), per retried
// list: an update in which the list had no sources (or no retry at all) tells nothing and is skipped
struct SvHist {
  enum { LARGE = 0, MID = 1, MULTI = 2, NLIST = 3 };
  int seen[NLIST] = {0, 0, 0};
  int64_t prev1[NLIST] = {0, 0, 0};
  int64_t prev2[NLIST] = {0, 0, 0};
  int64_t cnt1[NLIST] = {0, 0, 0};  // the list's class size at the last update (sv_scale_prev)
  void push(int list, int64_t first, int64_t cnt) {
    prev2[list] = prev1[list];
    prev1[list] = first;
    cnt1[list] = cnt;
    seen[list]++;
  }
  // the grid of the list's next retry launch behind a class of `cnt` sources
  int64_t grid(int list, int64_t cnt, int mode) const {
    return sv_retry_grid(cnt, seen[list], sv_scale_prev(prev1[list], cnt1[list], cnt), prev2[list], mode);
  }
};

}  // namespace pprk
