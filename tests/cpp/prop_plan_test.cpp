// Host planning of the transposed feature propagation (csrc/prop_plan.h), as a program of its own:
// the key-range cutter, the chunk-task builder, the column blocks and the weight rule (W == 0
// included: GRank cannot produce an all-zero row, so the device tests cannot cover it).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../approximated_personalized_pagerank_amd/csrc/prop_plan.h"

using namespace pprprop;

static int checks = 0;
#define CHECK(x)                                                    \
  do {                                                              \
    checks++;                                                       \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                     \
    }                                                               \
  } while (0)

// the ranges partition [0, n), hold at most E postings unless they are a single key, and are maximal
static int check_ranges(const std::vector<int32_t>& cnt, int64_t E) {
  const int64_t n = (int64_t)cnt.size();
  const std::vector<KeyRange> r = cut_key_ranges(cnt.data(), n, E);
  CHECK((n == 0) == r.empty());
  int64_t k = 0;
  for (size_t i = 0; i < r.size(); i++) {
    CHECK(r[i].k0 == k && r[i].k1 > r[i].k0 && r[i].k1 <= n);
    int64_t sum = 0;
    for (int64_t q = r[i].k0; q < r[i].k1; q++) sum += cnt[(size_t)q];
    CHECK(sum == r[i].postings);
    CHECK(sum <= E || r[i].k1 - r[i].k0 == 1);
    if (i + 1 < r.size()) CHECK(sum + cnt[(size_t)r[i].k1] > E);  // the next key did not fit
    k = r[i].k1;
  }
  CHECK(k == n);
  return 0;
}

// every posting lies in exactly one task, in order; chunks are full but the last; partial rows are
// consecutive per key and folds name them
static int check_tasks(const std::vector<int32_t>& cnt, int64_t k0, int chunk) {
  const int64_t nk = (int64_t)cnt.size();
  std::vector<int32_t> start((size_t)nk + 1, 0);
  for (int64_t k = 0; k < nk; k++) start[(size_t)k + 1] = start[(size_t)k] + cnt[(size_t)k];
  ChunkPlan p;
  p.tasks.push_back(PTask{1, 2, 3, 4});  // (stale contents are dropped)
  build_chunk_tasks(start.data(), nk, k0, chunk, p);
  size_t t = 0, f = 0;
  int64_t parts = 0, zero = 0;
  for (int64_t k = 0; k < nk; k++) {
    const int64_t c = cnt[(size_t)k];
    if (c == 0) { zero++; continue; }
    const int64_t m = (c + chunk - 1) / chunk;
    if (m > 1) {
      CHECK(f < p.folds.size());
      CHECK(p.folds[f].key == k0 + k && p.folds[f].m == m && p.folds[f].part == parts);
      f++;
    }
    for (int64_t j = 0; j < m; j++, t++) {
      CHECK(t < p.tasks.size());
      const PTask& x = p.tasks[t];
      CHECK(x.key == k0 + k);
      CHECK(x.off == start[(size_t)k] + j * chunk);
      CHECK(x.n == (j + 1 < m ? chunk : c - j * chunk) && x.n >= 1 && x.n <= chunk);
      CHECK(x.part == (m > 1 ? parts++ : -1));
    }
  }
  CHECK(t == p.tasks.size() && f == p.folds.size() && parts == p.nparts && zero == p.nzero);
  return 0;
}

int main() {
  // ---- the weight rule
  CHECK(prop_weight(0.25, 0.5) == 0.5);
  CHECK(prop_weight(0.25, 0.0) == 0.0);  // W == 0: every weight 0, no division
  CHECK(prop_weight(0.0, 0.0) == 0.0);
  {
    const double s[4] = {0.1, 0.2, 0.3, 1e-20};
    CHECK(prop_row_sum(s, 4) == ((0.0 + 0.1) + 0.2) + 0.3 + 1e-20);
    CHECK(prop_row_sum(s, 0) == 0.0);
    const double z[3] = {0.0, 0.0, 0.0};
    const double W = prop_row_sum(z, 3);
    CHECK(W == 0.0);
    for (double x : z) CHECK(prop_weight(x, W) == 0.0);
  }
  // ---- key ranges
  if (check_ranges({}, 10)) return 1;
  if (check_ranges({0, 0, 0}, 10)) return 1;
  if (check_ranges({5, 5, 5, 5}, 10)) return 1;
  if (check_ranges({11, 1, 30, 0, 0, 2}, 10)) return 1;  // keys wider than E stand alone
  if (check_ranges({1, 2, 3}, 0)) return 1;              // E below 1 is read as 1
  {
    const std::vector<int32_t> c = {3, 3, 3, 3};
    CHECK(cut_key_ranges(c.data(), 4, 100).size() == 1);
    CHECK(cut_key_ranges(c.data(), 4, 6).size() == 2);
    CHECK(cut_key_ranges(c.data(), 4, 3).size() == 4);
  }
  std::mt19937 rng(7);
  for (int rep = 0; rep < 200; rep++) {
    std::vector<int32_t> c((size_t)(rng() % 300));
    for (int32_t& x : c) x = (rng() % 4 == 0) ? (int32_t)(rng() % 3000) : (int32_t)(rng() % 3);
    if (check_ranges(c, 1 + (int64_t)(rng() % 4000))) return 1;
    if (check_tasks(c, (int64_t)(rng() % 1000), 1 + (int)(rng() % 600))) return 1;
    if (check_tasks(c, 0, PROP_CHUNK)) return 1;
  }
  // ---- chunk boundaries
  if (check_tasks({512}, 0, PROP_CHUNK)) return 1;
  if (check_tasks({513}, 5, PROP_CHUNK)) return 1;
  if (check_tasks({1, 0, 1024, 1025, 0}, 9, PROP_CHUNK)) return 1;
  {
    const int32_t bad[3] = {4, 2, 2};  // a decreasing pair reads as an empty list
    ChunkPlan p;
    build_chunk_tasks(bad, 2, 0, PROP_CHUNK, p);
    CHECK(p.tasks.empty() && p.nzero == 2);
  }
  // ---- column blocks
  CHECK(prop_col_block(0, 100, 64, 1 << 20) == 128);
  CHECK(prop_col_block(1, 100, 64, 1 << 20) == 128);
  CHECK(prop_col_block(1024, 8192, 256, 1 << 20) == 256);       // never below one tile
  CHECK(prop_col_block(16, 8192, 256, 16 * 8 * 1024) == 1024);  // budget / (8 nparts), whole tiles
  CHECK(prop_col_block(16, 8192, 256, 16 * 8 * 1100) == 1024);
  std::printf("ok %d\n", checks);
  return 0;
}
