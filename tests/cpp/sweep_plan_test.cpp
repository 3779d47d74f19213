// sweep_plan_test.cpp -- the host planning of the sweep cuts (csrc/sweep_plan.h) on its own: the tier
// rule partitions the sources, slices cover [0, W) once and in order, batches and chunks respect
// their budgets, the refusals come in their order, and the exact ratio comparison agrees with
// __int128. Pure host code: compiled with g++ -fsanitize=address,undefined by
// tests/test_sweep_plan_host.py and run as a program.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../approximated_personalized_pagerank_amd/csrc/sweep_plan.h"

using namespace pprsweep;

static long checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    checks++;                                                           \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static void test_tiers(std::mt19937_64& rng) {
  const int64_t ws[] = {0, 1, 63, 64, 2047, 2048, 2049, 1 << 17, (1 << 17) + 1, (int64_t)1 << 30, ((int64_t)1 << 30) + 1,
                        (int64_t)1 << 40};
  const int members[] = {0, 1, 64, 191, 192, 193, 768, 769, 1536, 3072, 3073, 4096};
  const int64_t knobs[] = {0, 1, 2048, 1 << 17, (int64_t)1 << 30};
  for (int64_t wm : knobs)
    for (int64_t gm : knobs)
      for (int64_t W : ws)
        for (int mem : members) {
          const int code = sw_tier(W, mem, clamp_wave_max(wm), clamp_wg_max(gm));
          const bool wave = code == SW_CODE_WAVE, slice = code == SW_CODE_SLICE;
          const bool wg = code > SW_CODE_WG && code < SW_CODE_SLICE;
          CHECK((int)wave + (int)wg + (int)slice == 1);
          if (wave) CHECK(wm > 0 && W <= wm && 4 * mem <= 3 * SW_WAVE_T);
          if (wg) {
            const int T = 1 << (code - SW_CODE_WG);
            CHECK(gm > 0 && W <= gm && T >= SW_MIN_T && T <= SW_MAX_T && 4 * (int64_t)mem <= 3 * (int64_t)T);
            CHECK(T == sw_table_slots(mem) && (T == SW_MIN_T || 4 * (int64_t)mem > 3 * (int64_t)(T / 2)));
            CHECK(!(wm > 0 && W <= wm && 4 * mem <= 3 * SW_WAVE_T));
          }
          if (slice) CHECK(!(gm > 0 && W <= gm) && !(wm > 0 && W <= wm && 4 * mem <= 3 * SW_WAVE_T));
        }
  CHECK(clamp_wave_max(-5) == 0 && clamp_wg_max(((int64_t)1 << 40)) == SW_EDGE_LIMIT);
  CHECK(clamp_slice(0) == 64 && clamp_slice(1024) == 1024 && clamp_slice((int64_t)1 << 50) == SW_EDGE_LIMIT);
  for (int i = 0; i < 2000; i++) {
    const int mem = (int)(rng() % 4097);
    const int T = sw_table_slots(mem);
    CHECK((T & (T - 1)) == 0 && 4 * (int64_t)mem <= 3 * (int64_t)T && (1 << sw_log2(T)) == T);
  }
}

static void test_slices(std::mt19937_64& rng) {
  std::vector<STask> tasks;
  std::vector<SBatch> batches;
  for (int trial = 0; trial < 300; trial++) {
    const int64_t count = (int64_t)(rng() % 40);
    const int64_t slice = 1 + (int64_t)(rng() % (trial % 3 ? 5000 : 7));
    const int64_t budget = trial % 5 == 0 ? 0 : 1 + (int64_t)(rng() % 9);
    std::vector<int32_t> list((size_t)count);
    std::vector<int64_t> W((size_t)count);
    for (int64_t i = 0; i < count; i++) {
      list[(size_t)i] = (int32_t)(rng() % 100000);
      W[(size_t)i] = trial % 7 == 0 ? 0 : (int64_t)(rng() % 20000);
    }
    cut_slices(list.data(), W.data(), count, slice, budget, tasks, batches);
    const int64_t rows = budget < 1 ? 1 : budget;
    int64_t next_r = 0, next_t = 0;
    for (const SBatch& b : batches) {
      CHECK(b.r0 == next_r && b.t0 == next_t && b.r1 > b.r0 && b.r1 - b.r0 <= rows && b.t1 > b.t0);
      int64_t t = b.t0;
      for (int64_t r = b.r0; r < b.r1; r++) {  // the slices of one source: consecutive, in order, covering [0, W)
        int64_t e = 0;
        bool first = true;
        while (t < b.t1 && tasks[(size_t)t].row == (int32_t)(r - b.r0) && (first || e < W[(size_t)r])) {
          const STask& k = tasks[(size_t)t];
          CHECK(k.q == list[(size_t)r] && k.e0 == e && k.e1 >= k.e0 && k.e1 - k.e0 <= slice && k.e1 <= W[(size_t)r]);
          CHECK(k.e1 == W[(size_t)r] || k.e1 - k.e0 == slice);
          e = k.e1;
          first = false;
          t++;
        }
        CHECK(!first && e == W[(size_t)r]);
      }
      CHECK(t == b.t1);
      next_r = b.r1;
      next_t = b.t1;
    }
    CHECK(next_r == count && next_t == (int64_t)tasks.size());
  }
}

static void test_chunks(std::mt19937_64& rng) {
  for (int trial = 0; trial < 500; trial++) {
    const int64_t rows = (int64_t)(rng() % 5000), width = (int64_t)(rng() % 4097);
    const int64_t chunk = (int64_t)(rng() % 300) - 5, budget = (int64_t)(rng() % 200000);
    const std::vector<int64_t> b = cut_chunks(rows, width, chunk, budget);
    CHECK(!b.empty() && b.front() == 0 && b.back() == rows);
    for (size_t i = 0; i + 1 < b.size(); i++) {
      const int64_t nq = b[i + 1] - b[i];
      CHECK(nq >= 1 && nq <= (chunk < 1 ? 1 : chunk));
      CHECK(nq == 1 || nq * width <= budget);
    }
    if (rows == 0) CHECK(b.size() == 1);
  }
}

static void test_refusals() {
  const int64_t n = 100, m = 1000;
  auto ck = [&](bool plan_ok, int64_t rows, bool ids, bool vec, int64_t rw, uint32_t mn, uint32_t mx, int64_t mv, uint32_t fl,
                bool outs, bool pc, bool pv) { return check_sweep_args(plan_ok, n, m, rows, ids, vec, rw, mn, mx, mv, fl, outs, pc, pv); };
  CHECK(ck(true, 3, true, false, 32, 1, 0, 0, 0, true, false, false) == PPR_OK);
  CHECK(ck(true, n, false, false, 32, 1, 0, 0, 0, true, true, true) == PPR_OK);
  CHECK(ck(true, 0, true, false, 32, 1, 0, 0, 0, false, false, false) == PPR_OK);  // no outputs needed for no rows
  CHECK(ck(true, 3, true, false, 32, 32, 0, m, 0, true, false, false) == PPR_OK);
  CHECK(ck(true, 3, true, false, 32, 40, 40, m, 0, true, false, false) == PPR_OK);  // max_size above L is a width
  CHECK(ck(true, 3, true, true, 32, 32, 4096, m, 0, true, false, false) == PPR_OK);  // vectors: width stays width_in
  // each refusal alone
  CHECK(ck(false, 3, true, false, 32, 1, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, -1, true, false, 32, 1, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, n - 1, false, false, 32, 1, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 2, false, true, 32, 1, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 1, 0, 0, 4, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 1, 0, 0, 0, true, true, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 1, 0, 0, 0, true, false, true) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 1, 0, 0, 0, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, -1, 1, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 1, 4097, 0, 0, true, false, false) == PPR_ERR_RANGE);
  CHECK(ck(true, 3, true, true, 4097, 1, 0, 0, 0, true, false, false) == PPR_ERR_RANGE);
  CHECK(ck(true, 3, true, false, 32, 0, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 33, 0, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 6, 5, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 32, 33, 4096, 0, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 1, 0, 0, 0, true, false, false) == PPR_ERR_ARG);  // (no width holds min_size 1)
  CHECK(ck(true, 3, true, false, 32, 1, 0, -1, 0, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 32, 1, 0, m + 1, 0, true, false, false) == PPR_ERR_ARG);
  // the order: a call wrong in two ways gets the code of the first check
  CHECK(ck(false, 3, true, false, 32, 1, 4097, 0, 0, true, false, false) == PPR_ERR_ARG);   // plan before range
  CHECK(ck(true, 3, true, false, 32, 1, 4097, 0, 1, true, false, false) == PPR_ERR_ARG);    // flags before range
  CHECK(ck(true, 3, true, false, 32, 1, 4097, 0, 0, true, true, false) == PPR_ERR_ARG);     // profiles before range
  CHECK(ck(true, 3, true, false, 32, 1, 4097, 0, 0, false, false, false) == PPR_ERR_ARG);   // outputs before range
  CHECK(ck(true, 3, true, false, 32, 0, 4097, 0, 0, true, false, false) == PPR_ERR_RANGE);  // range before min_size
  CHECK(ck(true, 3, true, false, 32, 0, 4097, -1, 0, true, false, false) == PPR_ERR_RANGE); // ... and before max_vol
  // sources and vectors
  const int32_t good[] = {0, 99, 5, 5}, bad_hi[] = {0, 100}, bad_lo[] = {3, -1};
  CHECK(check_sources(good, 4, n) == PPR_OK && check_sources(bad_hi, 2, n) == PPR_ERR_SOURCE);
  CHECK(check_sources(bad_lo, 2, n) == PPR_ERR_SOURCE && check_sources(bad_lo, 1, n) == PPR_OK);
  CHECK(check_sources(nullptr, 0, n) == PPR_OK);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  int32_t ids[8] = {5, 9, 2, 777, 7, 1, 7, -5};  // (entries past a row's length are never read as ids)
  double sc[8] = {0.5, 0.25, 0.0, nan, 0.5, 0.5, -1.0, inf};
  int32_t len[2] = {3, 2};
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_OK);
  CHECK(check_vectors(0, 4, nullptr, nullptr, nullptr, n) == PPR_OK);
  len[1] = 3;  // the repeated 7 and its negative score come into the row: the score is met first
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);
  sc[6] = 0.0;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);  // now the repeat
  ids[6] = 8;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_OK);
  len[0] = 4;  // NaN before the id 777 out of range
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);
  sc[3] = 1.0;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_SOURCE);
  ids[3] = 5;  // in range, repeated
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);
  ids[3] = 6;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_OK);
  len[1] = 5;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);
  len[1] = -1;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);
  len[1] = 4;  // inf, and -5
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_ARG);
  sc[7] = 3.0;
  CHECK(check_vectors(2, 4, ids, sc, len, n) == PPR_ERR_SOURCE);
  CHECK(sweep_width(0, 128, false) == 128 && sweep_width(7, 128, false) == 7 && sweep_width(4096, 128, false) == 4096);
  CHECK(sweep_width(0, 128, true) == 128 && sweep_width(7, 128, true) == 7 && sweep_width(4096, 128, true) == 128);
}

static void test_frac(std::mt19937_64& rng) {
  auto ref = [](int64_t ca, int64_t da, int64_t cb, int64_t db) {
    return (unsigned __int128)ca * (unsigned __int128)db < (unsigned __int128)cb * (unsigned __int128)da;
  };
  const int64_t big = (int64_t)1 << 62;
  const int64_t ext[] = {0, 1, 2, 3, 0xffffffffll, 0x100000000ll, 0x100000001ll, big - 1, big, big + 1,
                         std::numeric_limits<int64_t>::max() - 1, std::numeric_limits<int64_t>::max()};
  for (int64_t ca : ext)
    for (int64_t da : ext)
      for (int64_t cb : ext)
        for (int64_t db : ext) {
          if (da == 0 || db == 0) continue;
          CHECK(frac_less(ca, da, cb, db) == ref(ca, da, cb, db));
        }
  for (int i = 0; i < 200000; i++) {
    const int sh = (int)(rng() % 63);
    int64_t v[4];
    for (int64_t& x : v) x = (int64_t)((rng() >> 1) >> (rng() % 2 ? sh : (int)(rng() % 63)));
    if (i % 3 == 0) { v[1] = big - (int64_t)(rng() % 1000); v[3] = big - (int64_t)(rng() % 1000); }  // dens near 2^62
    if (i % 5 == 0) { v[2] = v[0]; v[3] = v[1]; }                                                    // equal ratios
    if (i % 7 == 0 && v[1] < big && v[0] < big) { v[2] = 2 * v[0]; v[3] = 2 * v[1]; }                // equal, not identical
    if (v[1] == 0 || v[3] == 0) continue;
    CHECK(frac_less(v[0], v[1], v[2], v[3]) == ref(v[0], v[1], v[2], v[3]));
    const U128 p = mul64((uint64_t)v[0], (uint64_t)v[3]);
    const unsigned __int128 q = (unsigned __int128)(uint64_t)v[0] * (uint64_t)v[3];
    CHECK(p.lo == (uint64_t)q && p.hi == (uint64_t)(q >> 64));
  }
  const U128 top = mul64(~0ull, ~0ull);
  CHECK(top.lo == 1ull && top.hi == ~0ull - 1ull);
}

int main() {
  std::mt19937_64 rng(12345);
  test_tiers(rng);
  test_slices(rng);
  test_chunks(rng);
  test_refusals();
  test_frac(rng);
  std::printf("ok %ld\n", checks);
  return 0;
}
