// The sieve's retry-grid rule (csrc/sv_plan.h), stand-alone under ASan + UBSan
// (tests/test_sv_retry_grid_host.py). Prints "ok <checks>" and exits 0, or the failed check and 1.
#include <cstdio>

#include "../../approximated_personalized_pagerank_amd/csrc/sv_plan.h"

using namespace pprk;

static int checks = 0, bad = 0;
#define CHECK_EQ(expr, want)                                                                  \
  do {                                                                                        \
    const long long got_ = (long long)(expr), want_ = (long long)(want);                      \
    checks++;                                                                                 \
    if (got_ != want_) {                                                                      \
      bad++;                                                                                  \
      std::fprintf(stderr, "%s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #expr, got_, want_); \
    }                                                                                         \
  } while (0)

int main() {
  const int A = SV_GRID_AUTO;
  // first update of the partition: the whole class, whatever the (unset) history says
  CHECK_EQ(sv_retry_grid(8800, 0, 0, 0, A), 8800);
  CHECK_EQ(sv_retry_grid(1, 0, 0, 0, A), 1);
  CHECK_EQ(sv_retry_grid(11000, 0, 5, 7, A), 11000);
  // later updates: 2 prev1 + 64, at most the class
  CHECK_EQ(sv_retry_grid(11000, 1, 8846, 0, A), 11000);
  CHECK_EQ(sv_retry_grid(11000, 1, 1514, 0, A), 2 * 1514 + 64);
  CHECK_EQ(sv_retry_grid(11000, 2, 100, 8846, A), 264);
  CHECK_EQ(sv_retry_grid(11000, 5, 1, 0, A), 66);
  CHECK_EQ(sv_retry_grid(50, 5, 1, 0, A), 50);
  CHECK_EQ(sv_retry_grid(11000, 3, 0, 9, A), 64);   // one zero is not two
  CHECK_EQ(sv_retry_grid(11000, 1, 0, 0, A), 64);   // ... nor is a second update's unset prev2
  // two updates without an overflow: no launch
  CHECK_EQ(sv_retry_grid(11000, 2, 0, 0, A), 0);
  CHECK_EQ(sv_retry_grid(11000, 14, 0, 0, A), 0);
  // ... until one is counted again
  CHECK_EQ(sv_retry_grid(11000, 15, 3, 0, A), 70);
  // an empty class has no launch in any mode
  CHECK_EQ(sv_retry_grid(0, 0, 0, 0, A), 0);
  CHECK_EQ(sv_retry_grid(0, 3, 9, 9, SV_GRID_FULL), 0);
  CHECK_EQ(sv_retry_grid(0, 3, 9, 9, SV_GRID_LEGACY), 0);
  CHECK_EQ(sv_retry_grid(0, 3, 9, 9, 5), 0);
  // no overflow of 2 prev1 + 64 at the largest counts
  CHECK_EQ(sv_retry_grid((int64_t)1 << 40, 4, (int64_t)1 << 38, 0, A), ((int64_t)1 << 39) + 64);
  // the override modes ignore the history
  for (int seen = 0; seen < 4; seen++) {
    CHECK_EQ(sv_retry_grid(11000, seen, 0, 0, SV_GRID_LEGACY), 11000 / 8 + 64);
    CHECK_EQ(sv_retry_grid(10, seen, 0, 0, SV_GRID_LEGACY), 10);
    CHECK_EQ(sv_retry_grid(11000, seen, 0, 0, SV_GRID_FULL), 11000);
    CHECK_EQ(sv_retry_grid(11000, seen, 9000, 9000, 1), 1);
    CHECK_EQ(sv_retry_grid(11000, seen, 0, 0, 300), 300);
    CHECK_EQ(sv_retry_grid(200, seen, 0, 0, 300), 200);
    CHECK_EQ(sv_retry_grid(200, seen, 50, 50, 0), 0);
  }
  // PPR_SV_RETRY_GRID
  CHECK_EQ(sv_retry_mode_parse(nullptr), SV_GRID_AUTO);
  CHECK_EQ(sv_retry_mode_parse(""), SV_GRID_AUTO);
  CHECK_EQ(sv_retry_mode_parse("auto"), SV_GRID_AUTO);
  CHECK_EQ(sv_retry_mode_parse("legacy"), SV_GRID_LEGACY);
  CHECK_EQ(sv_retry_mode_parse("full"), SV_GRID_FULL);
  CHECK_EQ(sv_retry_mode_parse("1"), 1);
  CHECK_EQ(sv_retry_mode_parse("4096"), 4096);
  CHECK_EQ(sv_retry_mode_parse("99999999999999"), 1 << 30);
  CHECK_EQ(sv_retry_mode_parse("-3"), SV_GRID_AUTO);
  CHECK_EQ(sv_retry_mode_parse("12x"), SV_GRID_AUTO);
  // the history shifts per list
  SvHist h;
  CHECK_EQ(h.seen[SvHist::LARGE], 0);
  h.push(SvHist::LARGE, 8846, 11000);
  h.push(SvHist::LARGE, 12, 11000);
  h.push(SvHist::MULTI, 3, 40);
  CHECK_EQ(h.seen[SvHist::LARGE], 2);
  CHECK_EQ(h.prev1[SvHist::LARGE], 12);
  CHECK_EQ(h.prev2[SvHist::LARGE], 8846);
  CHECK_EQ(h.seen[SvHist::MULTI], 1);
  CHECK_EQ(h.prev1[SvHist::MULTI], 3);
  CHECK_EQ(h.seen[SvHist::MID], 0);
  CHECK_EQ(h.cnt1[SvHist::LARGE], 11000);
  CHECK_EQ(h.grid(SvHist::LARGE, 11000, A), 2 * 12 + 64);
  CHECK_EQ(h.grid(SvHist::LARGE, 22000, A), 2 * 24 + 64);   // the class doubled: so does the count
  CHECK_EQ(h.grid(SvHist::LARGE, 5000, A), 2 * 12 + 64);    // a class that shrank keeps it
  CHECK_EQ(h.grid(SvHist::MULTI, 400, A), 2 * 30 + 64);
  CHECK_EQ(h.grid(SvHist::MID, 7, A), 7);                   // never updated: the whole class
  h.push(SvHist::LARGE, 0, 11000);
  h.push(SvHist::LARGE, 0, 11000);
  CHECK_EQ(h.grid(SvHist::LARGE, 100, A), 0);
  CHECK_EQ(h.grid(SvHist::LARGE, 1000000, A), 0);
  CHECK_EQ(h.grid(SvHist::LARGE, 100, SV_GRID_LEGACY), 76);
  h = SvHist{};
  CHECK_EQ(h.grid(SvHist::LARGE, 100, A), 100);
  // a first update of a few full-row sources, then the whole class: the grid follows the rate
  h.push(SvHist::LARGE, 300, 320);
  CHECK_EQ(h.grid(SvHist::LARGE, 5000, A), 5000);
  CHECK_EQ(sv_scale_prev(300, 320, 5000), 4688);
  CHECK_EQ(sv_scale_prev(300, 320, 320), 300);
  CHECK_EQ(sv_scale_prev(300, 320, 100), 300);
  CHECK_EQ(sv_scale_prev(0, 320, 5000), 0);
  CHECK_EQ(sv_scale_prev(-4, 320, 5000), 0);
  CHECK_EQ(sv_scale_prev(7, 0, 5000), 7);
  CHECK_EQ(sv_scale_prev(400, 320, 5000), 5000);            // (more overflows than sources: capped)
  CHECK_EQ(sv_scale_prev((int64_t)1 << 61, (int64_t)1 << 61, (int64_t)1 << 62), (int64_t)1 << 62);
  if (bad) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
