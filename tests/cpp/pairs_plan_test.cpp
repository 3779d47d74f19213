// pairs_plan_test.cpp -- the host planning of the node-pair scores (csrc/pairs_plan.h) on its own:
// the refusals come in their order, every group gets exactly one tier, the tasks of a split group
// cover its candidates once and in order, chunks respect their budgets and cover the call, the size
// checks hold at 2^31 - 1 and 2^62, the limb sums of the wave reduction equal unsigned __int128 sums,
// and the byte accounting gives the header's figures on hand-made groups. Pure host code: compiled
// with g++ -fsanitize=address,undefined by tests/test_pairs_plan_host.py and run as a program.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../approximated_personalized_pagerank_amd/csrc/pairs_plan.h"

using namespace pprpairs;

static long checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    checks++;                                                           \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static void test_refusals() {
  const int64_t ok[] = {0, 2, 2, 5}, bad0[] = {1, 2, 3, 4}, dec[] = {0, 3, 2, 5}, none[] = {0, 0, 0, 0};
  const uint32_t all = PR_FWD | PR_DOT;
  CHECK(check_pairs_args(true, 3, ok, true, true, 0, all) == PPR_OK);
  CHECK(check_pairs_args(true, 0, ok, false, false, 0, all) == PPR_OK);  // no group: no array is needed
  CHECK(check_pairs_args(true, 3, none, true, false, 0, PR_SLEN) == PPR_OK);  // no pair: no candidates
  // each refusal on its own
  CHECK(check_pairs_args(false, 3, ok, true, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, nullptr, true, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, -1, ok, true, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, bad0, true, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, dec, true, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, ok, false, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, ok, true, false, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, ok, true, true, 1, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, ok, true, true, 1u << 31, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, 3, ok, true, true, 0, 0) == PPR_ERR_ARG);
  // nothing is read through gptr before the plan, the pointer and Q are accepted
  CHECK(check_pairs_args(false, 1 << 20, ok, true, true, 0, all) == PPR_ERR_ARG);
  CHECK(check_pairs_args(true, -5, nullptr, true, true, 0, all) == PPR_ERR_ARG);
  // the order: PPR_ERR_ARG of every kind before PPR_ERR_RANGE, that before PPR_ERR_SOURCE
  const int64_t huge[] = {0, (int64_t)1 << 31};
  CHECK(check_pairs_args(true, 1, huge, true, true, 0, all) == PPR_OK);
  CHECK(check_pairs_sizes(1, huge[1]) == PPR_ERR_RANGE);
  CHECK(check_pairs_args(true, 1, huge, true, true, 2, all) == PPR_ERR_ARG);   // flags before the range
  CHECK(check_pairs_args(true, 1, huge, true, true, 0, 0) == PPR_ERR_ARG);     // no output before the range
  CHECK(check_pairs_args(true, 1, huge, true, false, 0, all) == PPR_ERR_ARG);  // null candidates before the range
  const int32_t ids[] = {0, 4, 9, 3}, neg[] = {0, -1}, big[] = {10};
  CHECK(check_ids(ids, 4, 10) == PPR_OK && check_ids(ids, 4, 9) == PPR_ERR_SOURCE && check_ids(neg, 2, 10) == PPR_ERR_SOURCE);
  CHECK(check_ids(big, 1, 10) == PPR_ERR_SOURCE && check_ids(big, 0, 10) == PPR_OK && check_ids(nullptr, 0, 10) == PPR_OK);
  // sizes at the edges, without overflow
  const int64_t m = 0x7fffffff;
  CHECK(check_pairs_sizes(m, m) == PPR_OK && check_pairs_sizes(m + 1, 0) == PPR_ERR_RANGE && check_pairs_sizes(0, m + 1) == PPR_ERR_RANGE);
  CHECK(check_pairs_sizes((int64_t)1 << 62, 0) == PPR_ERR_RANGE && check_pairs_sizes(0, (int64_t)1 << 62) == PPR_ERR_RANGE);
  CHECK(check_pairs_sizes(INT64_MAX, INT64_MAX) == PPR_ERR_RANGE && check_pairs_sizes(0, 0) == PPR_OK);
  // classes
  CHECK(pr_class(PR_FWD | PR_BWD | PR_HIT | PR_RANK | PR_SLEN | PR_CLEN) == PR_LOOKUP);
  CHECK(pr_class(PR_COMMON) == PR_OVERLAP && pr_class(PR_DOT) == PR_OVERLAP && pr_class(PR_FWD | PR_DOT) == PR_OVERLAP);
}

static void test_tiers() {
  const int64_t ns[] = {0, 1, 2, 3, 4, 15, 16, 17, 1023, 1024, 1025, 1 << 20, 0x7fffffff, (int64_t)1 << 62};
  const int64_t knobs[] = {-3, 0, 1, 3, 16, 1024, (int64_t)1 << 30, (int64_t)1 << 40};
  for (int64_t w0 : knobs)
    for (int64_t s0 : knobs)
      for (int64_t nc : ns) {
        const int64_t wm = clamp_wave_max(w0), sp = clamp_split(s0);
        CHECK(wm >= 0 && wm <= PR_MAX_COUNT && sp >= 1 && sp <= PR_CHUNK_PAIRS);
        const int t = pr_tier(nc, wm, sp);
        CHECK(t == PR_TIER_WAVE || t == PR_TIER_WG || t == PR_TIER_SPLIT);
        CHECK((t == PR_TIER_SPLIT) == (nc > sp));
        if (t == PR_TIER_WAVE) CHECK(wm > 0 && nc <= wm);
        if (t == PR_TIER_WG) CHECK(!(wm > 0 && nc <= wm));
      }
  CHECK(pr_tier(16, PR_WAVE_MAX_DEFAULT, PR_SPLIT_DEFAULT) == PR_TIER_WAVE && pr_tier(17, PR_WAVE_MAX_DEFAULT, PR_SPLIT_DEFAULT) == PR_TIER_WG);
  CHECK(pr_tier(1024, PR_WAVE_MAX_DEFAULT, PR_SPLIT_DEFAULT) == PR_TIER_WG && pr_tier(1025, PR_WAVE_MAX_DEFAULT, PR_SPLIT_DEFAULT) == PR_TIER_SPLIT);
  CHECK(pr_tier(0, 0, 1) == PR_TIER_WG && pr_tier(0, 1, 1) == PR_TIER_WAVE);
  CHECK(!pr_use_binary(PR_SEARCH_LINEAR, 4096) && pr_use_binary(PR_SEARCH_BINARY, 1));
  CHECK(!pr_use_binary(PR_SEARCH_AUTO, 128) && !pr_use_binary(PR_SEARCH_AUTO, 511) && pr_use_binary(PR_SEARCH_AUTO, 512));
  CHECK(clamp_chunk(0) == 1 && clamp_chunk(-9) == 1 && clamp_chunk((int64_t)1 << 40) == PR_MAX_COUNT);
}

// chunks cover the groups and the pairs in order within their budgets; the tasks of all chunks cover
// every candidate once, in order, within its group, in runs of at most `split`; every group is counted
// by exactly one tier
static void check_plan(const std::vector<int64_t>& gptr, int64_t chunk_groups, int64_t pair_budget, int64_t width,
                       int64_t entry_budget, int64_t wave_max, int64_t split) {
  const int64_t Q = (int64_t)gptr.size() - 1, P = gptr[Q];
  const std::vector<PChunk> ch = cut_chunks(Q, gptr.data(), chunk_groups, pair_budget, width, entry_budget);
  int64_t group_cap = std::max<int64_t>(1, chunk_groups);
  if (width > 0) group_cap = std::min(group_cap, std::max<int64_t>(1, entry_budget / width));
  int64_t q = 0, j = 0, tiers[3] = {0, 0, 0};
  std::vector<int> covered((size_t)P, 0);
  std::vector<PTask> wave, wg;
  CHECK(Q > 0 ? !ch.empty() : ch.empty());
  for (const PChunk& c : ch) {
    CHECK(c.j0 == j && c.j1 >= c.j0 && c.j1 - c.j0 <= std::max<int64_t>(1, pair_budget));
    CHECK(c.q0 <= c.q1 && c.q1 <= Q && c.q1 > c.q0);
    CHECK(c.q0 == q || c.q0 == q - 1);  // (the group the last chunk ended in may continue here)
    // the groups that start in the chunk are within the budget (one more may continue into it)
    CHECK(c.q1 - c.q0 <= group_cap + 1);
    // the chunk's pairs lie in its groups
    if (c.j1 > c.j0) CHECK(gptr[c.q0] <= c.j0 && c.j1 <= gptr[c.q1]);
    // a chunk either ends on a group boundary or is full
    CHECK(c.j1 == gptr[c.q1] || c.j1 - c.j0 == std::max<int64_t>(1, pair_budget) || c.q1 - c.q0 >= group_cap);
    cut_tasks(c, gptr.data(), wave_max, split, wave, wg, tiers);
    int64_t at = c.j0;  // tasks in order: wave and workgroup lists merged by position
    size_t iw = 0, ig = 0;
    while (iw < wave.size() || ig < wg.size()) {
      const bool takew = ig == wg.size() || (iw < wave.size() && wave[iw].j0 < wg[ig].j0);
      const PTask t = takew ? wave[iw++] : wg[ig++];
      CHECK(t.j0 < t.j1 && c.j0 + t.j0 >= at);
      // the gap before it holds no candidate
      CHECK(c.j0 + t.j0 == at);
      const int64_t g = c.q0 + t.g;
      CHECK(g >= c.q0 && g < c.q1 && gptr[g] <= c.j0 + t.j0 && c.j0 + t.j1 <= gptr[g + 1]);
      const int tier = pr_tier(gptr[g + 1] - gptr[g], wave_max, split);
      CHECK(takew == (tier == PR_TIER_WAVE));
      if (tier == PR_TIER_SPLIT) CHECK(t.j1 - t.j0 <= split); else CHECK(c.j0 + t.j0 == std::max(gptr[g], c.j0) && c.j0 + t.j1 == std::min(gptr[g + 1], c.j1));
      for (int64_t k = t.j0; k < t.j1; k++) covered[(size_t)(c.j0 + k)]++;
      at = c.j0 + t.j1;
    }
    CHECK(at == c.j1);
    j = c.j1;
    q = c.q1;
  }
  CHECK(j == P && q == Q);
  for (int64_t k = 0; k < P; k++) CHECK(covered[(size_t)k] == 1);
  CHECK(tiers[0] + tiers[1] + tiers[2] == Q);
  int64_t want[3] = {0, 0, 0};
  for (int64_t g = 0; g < Q; g++) want[pr_tier(gptr[g + 1] - gptr[g], wave_max, split)]++;
  CHECK(tiers[0] == want[0] && tiers[1] == want[1] && tiers[2] == want[2]);
}

static void test_chunks_and_tasks(std::mt19937_64& rng) {
  // hand-made: empty groups at both ends and in the middle, one group larger than a chunk
  const std::vector<int64_t> hand{0, 0, 0, 3, 3, 10, 40, 40, 41, 41, 41};
  for (int64_t cg : {1, 2, 3, 100})
    for (int64_t pb : {1, 4, 7, 30, 1000})
      for (int64_t wm : {0, 2, 1000})
        for (int64_t sp : {1, 3, 8, 1000}) {
          check_plan(hand, cg, pb, 0, 0, wm, sp);
          check_plan(hand, cg, pb, 64, 128, wm, sp);
        }
  check_plan({0}, 4, 4, 0, 0, 16, 1024);
  check_plan({0, 0}, 4, 4, 0, 0, 16, 1024);
  for (int rep = 0; rep < 300; rep++) {
    const int Q = (int)(rng() % 40);
    std::vector<int64_t> gptr{0};
    for (int q = 0; q < Q; q++) {
      const uint64_t r = rng() % 10;
      gptr.push_back(gptr.back() + (int64_t)(r < 3 ? 0 : r < 8 ? rng() % 6 : rng() % 90));
    }
    const int64_t cg = 1 + (int64_t)(rng() % 9), pb = 1 + (int64_t)(rng() % 50);
    const int64_t wm = (int64_t)(rng() % 8), sp = 1 + (int64_t)(rng() % 20);
    check_plan(gptr, cg, pb, rep % 2 ? 32 : 0, 96, wm, sp);
  }
}

static void test_limbs(std::mt19937_64& rng) {
  typedef unsigned __int128 u128;
  const u128 mask96 = (((u128)1) << 96) - 1;
  for (int rep = 0; rep < 12000; rep++) {
    const int nvals = 1 + (int)(rng() % 200);
    std::vector<u128> v((size_t)nvals);
    u128 want = 0;
    for (u128& x : v) {
      const int bits = rep % 7 == 0 ? 95 : 1 + (int)(rng() % 95);  // up to 95 bits: the largest term and total of the contract
      x = ((((u128)rng()) << 64) | (u128)rng()) & ((((u128)1) << bits) - 1);
      if (rep % 11 == 0) x = (((u128)1) << 95) - 1;  // all ones: every carry
      want += x;
    }
    // a random grouping: lanes accumulate some values each, the lanes are then added in a random tree
    const int lanes = 1 + (int)(rng() % 64);
    std::vector<Limbs> lane((size_t)lanes, Limbs{0, 0, 0});
    for (const u128 x : v) {
      Limbs& l = lane[(size_t)(rng() % (uint64_t)lanes)];
      l = pr_add(l, pr_split((unsigned long long)x, (uint32_t)(x >> 64)));
    }
    while (lane.size() > 1) {
      const size_t a = (size_t)(rng() % lane.size());
      size_t b = (size_t)(rng() % (lane.size() - 1));
      if (b >= a) b++;
      lane[a] = pr_add(lane[a], lane[b]);
      lane.erase(lane.begin() + (long)b);
    }
    unsigned long long lo;
    uint32_t hi;
    pr_join(lane[0], lo, hi);
    const u128 got = (((u128)hi) << 64) | (u128)lo;
    CHECK(got == (want & mask96));
    // split and join are inverse on one value
    pr_join(pr_split((unsigned long long)v[0], (uint32_t)(v[0] >> 64)), lo, hi);
    CHECK(((((u128)hi) << 64) | (u128)lo) == v[0]);
  }
  // 64 lanes of the largest limbs: no word overflows
  Limbs s{0, 0, 0};
  for (int i = 0; i < 64 * 64; i++) s = pr_add(s, Limbs{0xffffffffull, 0xffffffffull, 0x7fffffffull});
  CHECK(s.w0 == 4096ull * 0xffffffffull && s.w2 == 4096ull * 0x7fffffffull);
}

static void test_bytes() {
  const uint32_t all = PR_FWD | PR_BWD | PR_HIT | PR_RANK | PR_COMMON | PR_DOT | PR_SLEN | PR_CLEN;
  CHECK(pr_pair_out_bytes(all) == 8 + 8 + 1 + 4 + 4 + 8 + 4 && pr_group_out_bytes(all) == 4);
  CHECK(pr_pair_out_bytes(PR_FWD) == 8 && pr_pair_out_bytes(PR_SLEN) == 0 && pr_group_out_bytes(PR_FWD) == 0);
  // overlap class, by hand: two groups, rows of 10 and 7 entries; group 0 in two tasks; five pairs whose
  // candidate rows hold 3, 4, 5, 6 and 7 entries with 1, 2, 0, 3 and 7 common keys
  PCount c;
  c.pairs = 5; c.groups = 2; c.tasks = 3; c.task_entries = 10 + 10 + 7; c.cand_entries = 25; c.hits = 13; c.slen_entries = 17;
  CHECK(pr_algo_bytes(PR_OVERLAP, all, c) == 5 * (37 + 4) + 2 * (4 + 4) + 4 * 17 + 12 * 27 + 128 * 3 + 2 * 27 + 4 * 25 + 8 * 13);
  CHECK(pr_algo_bytes(PR_OVERLAP, PR_COMMON, c) == 5 * (4 + 4) + 2 * 4 + 4 * 17 + 12 * 27 + 128 * 3 + 4 * 25);
  // lookup class: segments of 9 ids probed in all, 4 hits (3 forward), ranks built for both groups
  PCount l;
  l.pairs = 5; l.groups = 2; l.cand_entries = 9; l.hits = 4; l.fwd_hits = 3; l.task_entries = 17; l.ranked_groups = 2;
  l.slen_entries = 17; l.clen_entries = 25;
  const uint32_t look = PR_FWD | PR_BWD | PR_HIT | PR_RANK | PR_SLEN | PR_CLEN;
  CHECK(pr_algo_bytes(PR_LOOKUP, look, l) == 5 * (25 + 4) + 2 * (4 + 4) + 4 * 17 + 5 * 12 + 4 * 9 + 8 * 4 + 4 * 25 + 14 * 17 + 128 * 2 + 2 * 3);
  l.task_entries = 0; l.ranked_groups = 0; l.fwd_hits = 0; l.slen_entries = 0; l.clen_entries = 0;
  CHECK(pr_algo_bytes(PR_LOOKUP, PR_FWD, l) == 5 * (8 + 4) + 2 * 4 + 5 * 12 + 4 * 9 + 8 * 4);
  PCount z;
  z.groups = 3;
  CHECK(pr_algo_bytes(PR_LOOKUP, PR_FWD, z) == 12 && pr_algo_bytes(PR_OVERLAP, PR_DOT, z) == 12);
}

int main() {
  std::mt19937_64 rng(20240607);
  test_refusals();
  test_tiers();
  test_chunks_and_tasks(rng);
  test_limbs(rng);
  test_bytes();
  std::printf("ok %ld\n", checks);
  return 0;
}
