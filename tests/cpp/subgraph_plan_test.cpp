// subgraph_plan_test.cpp -- the host planning of the induced subgraph batches (csrc/subgraph_plan.h)
// on its own: the tier rule partitions the sources, slices cover a source's groups once, in order and
// on group boundaries, a slice's walk numbers its groups as the unsliced walk does, chunks and batches
// respect their budgets, the refusals come in their order, and the capacity and index-type checks
// hold at the 2^31 and 2^62 edges. Pure host code: compiled with g++ -fsanitize=address,undefined by
// tests/test_subgraph_plan_host.py and run as a program.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <utility>

#include "../../approximated_personalized_pagerank_amd/csrc/subgraph_plan.h"

using namespace pprsubg;

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
  const int64_t ws[] = {0, 1, 63, 64, 2047, 2048, 2049, 1 << 17, (1 << 17) + 1, (int64_t)1 << 30, ((int64_t)1 << 30) + 1};
  const int members[] = {0, 1, 64, 191, 192, 193, 768, 769, 1536, 3072, 3073, 4096};
  const int64_t knobs[] = {0, 1, 2048, 1 << 17, (int64_t)1 << 30, (int64_t)1 << 40, -3};
  for (int64_t wm0 : knobs)
    for (int64_t gm0 : knobs)
      for (int64_t W : ws)
        for (int mem : members) {
          const int64_t wm = clamp_wave_max(wm0), gm = clamp_wg_max(gm0);
          CHECK(wm >= 0 && wm <= SG_EDGE_LIMIT && gm >= 0 && gm <= SG_EDGE_LIMIT);
          const int code = sg_tier(W, mem, wm, gm);
          const bool wave = code == SG_CODE_WAVE, slice = code == SG_CODE_SLICE;
          const bool wg = code > SG_CODE_WG && code < SG_CODE_SLICE;
          CHECK((int)wave + (int)wg + (int)slice == 1);
          if (wave) CHECK(wm > 0 && W <= wm && 4 * mem <= 3 * SG_WAVE_T);
          if (wg) {
            const int T = 1 << (code - SG_CODE_WG);
            CHECK(gm > 0 && W <= gm && T >= SG_MIN_T && T <= SG_MAX_T && 4 * (int64_t)mem <= 3 * (int64_t)T);
            CHECK(T == sg_table_slots(mem) && (T == SG_MIN_T || 4 * (int64_t)mem > 3 * (int64_t)(T / 2)));
            CHECK(!(wm > 0 && W <= wm && 4 * mem <= 3 * SG_WAVE_T));
          }
          if (slice) CHECK(!(gm > 0 && W <= gm) && !(wm > 0 && W <= wm && 4 * mem <= 3 * SG_WAVE_T));
          // the slice tier's table holds the members too
          CHECK(4 * (int64_t)mem <= 3 * (int64_t)sg_table_slots(mem));
        }
  for (int i = 0; i < 2000; i++) {
    const int mem = (int)(rng() % 4097);
    const int T = sg_table_slots(mem);
    CHECK((T & (T - 1)) == 0 && 4 * (int64_t)mem <= 3 * (int64_t)T && (1 << sg_log2(T)) == T);
  }
  CHECK(slice_groups(0) == 1 && slice_groups(63) == 1 && slice_groups(64) == 1 && slice_groups(1024) == 16);
  CHECK(slice_groups(-9) == 1 && slice_groups((int64_t)1 << 50) == SG_EDGE_LIMIT / 64);
  // degrees as the walk counts them
  CHECK(sg_eff_deg(-4, 0) == 0 && sg_eff_deg(7, 0) == 7 && sg_eff_deg(7, 7) == 7 && sg_eff_deg(8, 7) == 0);
  CHECK(sg_eff_deg(SG_EDGE_LIMIT, 0) == SG_EDGE_LIMIT && sg_eff_deg(SG_EDGE_LIMIT + 5, 0) == SG_EDGE_LIMIT + 1);
  CHECK(sg_eff_deg(std::numeric_limits<int64_t>::max(), 0) == SG_EDGE_LIMIT + 1);
  CHECK(sg_eff_deg(std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::max()) == SG_EDGE_LIMIT + 1);
  CHECK(sg_eff_deg(std::numeric_limits<int64_t>::min(), 1) == 0);
  // 4096 members at the clamp cannot overflow the walk size
  CHECK(4096 * (SG_EDGE_LIMIT + 1) > SG_EDGE_LIMIT && 4096 * (SG_EDGE_LIMIT + 1) < ((int64_t)1 << 43));
}

// the walk of groups [g0, g1) as the device does it: (group number, first edge, edges) of every group
static std::vector<std::pair<int64_t, std::pair<int64_t, int64_t>>> walk(const std::vector<int64_t>& deg, int64_t g0,
                                                                         int64_t g1) {
  std::vector<std::pair<int64_t, std::pair<int64_t, int64_t>>> out;
  int64_t gw = 0, ebefore = 0;
  const int members = (int)deg.size();
  for (int w0 = 0; w0 < members && gw < g1; w0 += SG_GROUP) {
    int64_t total = 0;
    for (int i = w0; i < members && i < w0 + SG_GROUP; i++) total += deg[(size_t)i];
    const int64_t ngw = sg_window_groups(total);
    const int64_t lo = g0 > gw ? g0 - gw : 0, hi = g1 - gw < ngw ? g1 - gw : ngw;
    for (int64_t gi = lo; gi < hi; gi++)
      out.push_back({gw + gi, {ebefore + gi * SG_GROUP, std::min<int64_t>(SG_GROUP, total - gi * SG_GROUP)}});
    gw += ngw;
    ebefore += total;
  }
  return out;
}

static void test_slices(std::mt19937_64& rng) {
  std::vector<GTask> tasks;
  for (int trial = 0; trial < 400; trial++) {
    const int64_t count = (int64_t)(rng() % 12);
    const int64_t per_task = trial % 9 == 0 ? 0 : 1 + (int64_t)(rng() % (trial % 3 ? 40 : 3));
    std::vector<int32_t> list((size_t)count);
    std::vector<int64_t> groups((size_t)count);
    std::vector<std::vector<int64_t>> degs((size_t)count);
    for (int64_t i = 0; i < count; i++) {
      list[(size_t)i] = (int32_t)(rng() % 100000);
      const int members = trial % 7 == 0 ? 0 : (int)(rng() % 200);
      for (int j = 0; j < members; j++) {
        const int kind = (int)(rng() % 4);
        degs[(size_t)i].push_back(sg_eff_deg(kind == 0 ? 0 : kind == 1 ? (int64_t)(rng() % 3) : (int64_t)(rng() % 700),
                                             trial % 5 == 0 ? 300 : 0));
      }
      groups[(size_t)i] = sg_groups(degs[(size_t)i].data(), members);
    }
    cut_slices(list.data(), groups.data(), count, per_task, tasks);
    const int64_t per = per_task < 1 ? 1 : per_task;
    size_t t = 0;
    for (int64_t i = 0; i < count; i++) {
      const std::vector<int64_t>& d = degs[(size_t)i];
      int64_t W = 0;
      for (int64_t x : d) W += x;
      // the unsliced walk: every group once, numbered 0 .. G - 1, its edges one behind the other
      const auto whole = walk(d, 0, std::numeric_limits<int64_t>::max());
      CHECK((int64_t)whole.size() == groups[(size_t)i]);
      int64_t edges = 0;
      for (size_t g = 0; g < whole.size(); g++) {
        CHECK(whole[g].first == (int64_t)g && whole[g].second.second >= 1 && whole[g].second.second <= SG_GROUP);
        CHECK(whole[g].second.first >= edges);  // (in order; a window's last group may be short)
        edges += whole[g].second.second;
      }
      CHECK(edges == W);
      // the slices: consecutive, in order, on group boundaries; their walks are the whole walk, cut
      int64_t g = 0;
      size_t at = 0;
      while (t < tasks.size() && tasks[t].q == list[(size_t)i] && g < groups[(size_t)i]) {
        const GTask& k = tasks[t];
        CHECK(k.g0 == g && k.g1 > k.g0 && k.g1 - k.g0 <= per && k.g1 <= groups[(size_t)i]);
        CHECK(k.g1 == groups[(size_t)i] || k.g1 - k.g0 == per);
        const auto part = walk(d, k.g0, k.g1);
        CHECK((int64_t)part.size() == k.g1 - k.g0);
        for (const auto& x : part) {
          CHECK(at < whole.size() && x == whole[at]);
          at++;
        }
        g = k.g1;
        t++;
      }
      CHECK(g == groups[(size_t)i] && at == whole.size());
    }
    CHECK(t == tasks.size());
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
  CHECK(cut_chunks(500, 32, 7, SG_CHUNK_ENTRIES).size() - 1 == (500 + 6) / 7);
  for (int trial = 0; trial < 500; trial++) {
    const int64_t count = (int64_t)(rng() % 300);
    const int64_t gb = 1 + (int64_t)(rng() % 5000), mb = 1 + (int64_t)(rng() % 3000);
    std::vector<int64_t> groups((size_t)count);
    std::vector<int32_t> members((size_t)count);
    for (int64_t i = 0; i < count; i++) {
      groups[(size_t)i] = trial % 4 == 0 ? 0 : (int64_t)(rng() % 2000);
      members[(size_t)i] = (int32_t)(rng() % 400);
    }
    const std::vector<int64_t> b = cut_batches(groups.data(), members.data(), count, gb, mb);
    CHECK(!b.empty() && b.front() == 0 && b.back() == count && (count > 0 || b.size() == 1));
    for (size_t i = 0; i + 1 < b.size(); i++) {
      CHECK(b[i + 1] > b[i]);
      int64_t g = 0, m = 0;
      for (int64_t q = b[i]; q < b[i + 1]; q++) {
        g += groups[(size_t)q];
        m += members[(size_t)q];
      }
      CHECK(b[i + 1] - b[i] == 1 || (g <= gb && m <= mb));
      if (i + 2 < b.size())  // a batch ends only where the next source would break a budget
        CHECK(g + groups[(size_t)b[i + 1]] > gb || m + members[(size_t)b[i + 1]] > mb);
    }
  }
}

static void test_refusals() {
  const int64_t n = 100;
  // plan_ok, S, sources, host ptrs, size, max_deg, flags, node_cap, edge_cap, nodes, rowptr, col, scores, row, eid
  auto ck = [&](bool ok, int64_t S, bool src, bool hp, uint32_t size, int64_t md, uint32_t fl, int64_t nc, int64_t ec, bool no,
                bool rp, bool co, bool sc, bool ro, bool ei) {
    return check_subg_args(ok, n, S, src, hp, size, md, fl, nc, ec, no, rp, co, sc, ro, ei);
  };
  CHECK(ck(true, 3, true, true, 0, 0, 0, 96, 500, true, true, true, true, true, true) == PPR_OK);
  CHECK(ck(true, n, false, true, 4096, 5, 3, 0, 0, true, true, true, false, false, false) == PPR_OK);
  CHECK(ck(true, 0, true, true, 0, 0, 0, 0, 0, false, false, false, false, false, false) == PPR_OK);  // count-only
  CHECK(ck(true, SG_MAX_SOURCES, true, true, 1, 0, 2, 0, 0, false, false, false, false, false, false) == PPR_OK);
  // each refusal alone
  CHECK(ck(false, 3, true, true, 0, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, false, 0, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, -1, true, true, 0, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, n - 1, false, true, 0, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 4, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 1u << 31, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, -1, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, -1, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 9, -1, true, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 9, 9, false, true, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 9, 9, true, false, true, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 9, 9, true, true, false, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 0, 0, false, false, false, true, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 0, 0, false, false, false, false, true, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 0, 0, false, false, false, false, false, true) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 1, 0, false, false, false, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 0, 0, 0, 0, 1, false, false, false, false, false, false) == PPR_ERR_ARG);
  CHECK(ck(true, 3, true, true, 4097, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_RANGE);
  CHECK(ck(true, SG_MAX_SOURCES + 1, true, true, 0, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_RANGE);
  // the order: a call wrong in two ways gets the code of the first check
  CHECK(ck(false, 3, true, true, 4097, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);   // plan before range
  CHECK(ck(true, 3, true, true, 4097, 0, 8, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);    // flags before range
  CHECK(ck(true, 3, true, true, 4097, -2, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);   // max_deg before range
  CHECK(ck(true, 3, true, true, 4097, 0, 0, 9, 9, true, false, true, false, false, false) == PPR_ERR_ARG);   // pointers before range
  CHECK(ck(true, n + 5, false, true, 4097, 0, 0, 9, 9, true, true, true, false, false, false) == PPR_ERR_ARG);
  const int32_t good[] = {0, 99, 5, 5}, bad_hi[] = {0, 100}, bad_lo[] = {3, -1};
  CHECK(check_sources(good, 4, n) == PPR_OK && check_sources(bad_hi, 2, n) == PPR_ERR_SOURCE);
  CHECK(check_sources(bad_lo, 2, n) == PPR_ERR_SOURCE && check_sources(bad_lo, 1, n) == PPR_OK);
  CHECK(check_sources(nullptr, 0, n) == PPR_OK);
  CHECK(sg_width(0, 128) == 128 && sg_width(7, 128) == 7 && sg_width(4096, 128) == 4096);
}

static void test_capacity() {
  const int64_t i31 = ((int64_t)1 << 31) - 1, big = (int64_t)1 << 62, top = std::numeric_limits<int64_t>::max();
  CHECK(sg_index_limit(false) == i31 && sg_index_limit(true) == top);
  // the index type: 2^31 - 1 elements are numbered by int32, 2^31 are not
  CHECK(sg_capacity(i31, i31, i31, i31, false, false) == PPR_OK);
  CHECK(sg_capacity(i31 + 1, 5, top, top, false, false) == PPR_ERR_RANGE);
  CHECK(sg_capacity(5, i31 + 1, top, top, false, false) == PPR_ERR_RANGE);
  CHECK(sg_capacity(5, i31 + 1, 0, 0, false, true) == PPR_ERR_RANGE);   // count-only too
  CHECK(sg_capacity(i31 + 1, i31 + 1, top, top, true, false) == PPR_OK);
  CHECK(sg_capacity(big, big, big, big, true, false) == PPR_OK && sg_capacity(big, big + 1, big, big, true, false) == PPR_ERR_RANGE);
  CHECK(sg_capacity(top, top, top, top, true, false) == PPR_OK && sg_capacity(top, top, 0, 0, true, true) == PPR_OK);
  CHECK(sg_capacity(big, big, top, top, false, false) == PPR_ERR_RANGE);
  // the capacities
  CHECK(sg_capacity(10, 20, 10, 20, false, false) == PPR_OK && sg_capacity(10, 20, 9, 20, false, false) == PPR_ERR_RANGE);
  CHECK(sg_capacity(10, 20, 10, 19, false, false) == PPR_ERR_RANGE && sg_capacity(10, 20, 0, 0, false, true) == PPR_OK);
  CHECK(sg_capacity(0, 0, 0, 0, false, false) == PPR_OK);
  // the running check of the emit pass
  CHECK(sg_edges_fit(20, 20, false) && !sg_edges_fit(21, 20, false) && sg_edges_fit(0, 0, false));
  CHECK(sg_edges_fit(i31, top, false) && !sg_edges_fit(i31 + 1, top, false) && sg_edges_fit(i31 + 1, top, true));
  CHECK(sg_edges_fit(big, big, true) && !sg_edges_fit(big + 1, big, true) && sg_edges_fit(top, top, true));
}

int main() {
  std::mt19937_64 rng(4711);
  test_tiers(rng);
  test_slices(rng);
  test_chunks(rng);
  test_refusals();
  test_capacity();
  std::printf("ok %ld\n", checks);
  return 0;
}
