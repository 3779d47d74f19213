// What a resident-basket call decides before it touches the device (csrc/resident_args.h), as a
// program of its own: every refusal of a weighted CSR of id sets, which code wins when a call is
// wrong in two ways, the factors bit for bit, the slot rule, the power of two that holds Kq, and the
// host side of hash32 (the kernels probe with it tables the host builds with it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../approximated_personalized_pagerank_amd/csrc/resident_args.h"

using namespace pprres;

static int checks = 0;
#define CHECK(x)                                                    \
  do {                                                              \
    checks++;                                                       \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                     \
    }                                                               \
  } while (0)

static const uint32_t MAXK = 4096, FLAG = 1u;
static const int64_t N = 10;

// one call with everything sound unless overridden
struct Call {
  bool call_ok = true, outs_ok = true;
  int64_t n = N;
  std::vector<int64_t> qptr{0, 2, 3};
  std::vector<int32_t> ids{1, 2, 9};
  std::vector<double> w{1.0, 3.0, 5.0};
  bool has_qptr = true, has_ids = true, has_w = true;
  int64_t Q = 2;
  uint32_t Kq = 8, flags = 0;
  std::vector<double> fac;
  int run() {
    return check_weighted_sets(call_ok, n, Q, has_qptr ? qptr.data() : nullptr, has_ids ? ids.data() : nullptr,
                               has_w ? w.data() : nullptr, outs_ok, Kq, MAXK, flags, FLAG, fac);
  }
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static int test_refusals() {
  { Call c; CHECK(c.run() == PPR_OK); }
  // ---- every refusal, one case each
  { Call c; c.call_ok = false; CHECK(c.run() == PPR_ERR_ARG); }             // no plan / MC plan / iteration < 0
  { Call c; c.Q = -1; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.has_qptr = false; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.outs_ok = false; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.flags = 2u; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.flags = FLAG; CHECK(c.run() == PPR_OK); }
  { Call c; c.Kq = 0; CHECK(c.run() == PPR_ERR_K); }
  { Call c; c.Kq = MAXK + 1; CHECK(c.run() == PPR_ERR_RANGE); }
  { Call c; c.Kq = MAXK; CHECK(c.run() == PPR_OK); }
  { Call c; c.qptr = {1, 2, 3}; CHECK(c.run() == PPR_ERR_ARG); }            // qptr[0] != 0
  { Call c; c.qptr = {0, 3, 2}; CHECK(c.run() == PPR_ERR_ARG); }            // not monotone
  { Call c; c.has_ids = false; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.ids[1] = -1; CHECK(c.run() == PPR_ERR_SOURCE); }
  { Call c; c.ids[2] = (int32_t)N; CHECK(c.run() == PPR_ERR_SOURCE); }
  { Call c; c.ids[2] = (int32_t)N - 1; CHECK(c.run() == PPR_OK); }
  { Call c; c.w[0] = -1.0; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.w[0] = std::nan(""); CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.w[2] = std::numeric_limits<double>::infinity(); CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.w = {1e308, 1e308, 1.0}; CHECK(c.run() == PPR_ERR_ARG); }      // finite weights, W overflows
  { Call c; c.w = {0.0, 0.0, 1.0}; CHECK(c.run() == PPR_ERR_ARG); }          // all-zero weights of a non-empty query
  { Call c; c.w = {0.0, 2.0, 1.0}; CHECK(c.run() == PPR_OK); CHECK(c.fac[0] == 0.0 && c.fac[1] == 1.0); }
  // ---- precedence: wrong in two ways, the earlier check decides
  { Call c; c.Kq = 0; c.flags = 2u; CHECK(c.run() == PPR_ERR_ARG); }         // flags before K
  { Call c; c.Kq = 0; c.ids[0] = 99; CHECK(c.run() == PPR_ERR_K); }          // K before the ids
  { Call c; c.ids[0] = 99; c.w[1] = std::nan(""); CHECK(c.run() == PPR_ERR_SOURCE); }  // ids before the weights
  { Call c; c.qptr = {0, 3, 2}; c.has_ids = false; CHECK(c.run() == PPR_ERR_ARG); }    // monotone before the ids pointer
  { Call c; c.call_ok = false; c.Kq = 0; CHECK(c.run() == PPR_ERR_ARG); }    // the plan before everything
  { Call c; c.outs_ok = false; c.Kq = 0; CHECK(c.run() == PPR_ERR_ARG); }    // outputs before K
  { Call c; c.Kq = 0; c.qptr = {1, 2, 3}; CHECK(c.run() == PPR_ERR_K); }     // K before qptr[0]
  { Call c; c.Kq = MAXK + 1; c.qptr = {1, 2, 3}; CHECK(c.run() == PPR_ERR_RANGE); }
  { Call c; c.Kq = MAXK + 1; c.ids[0] = -5; CHECK(c.run() == PPR_ERR_RANGE); }
  { Call c; c.qptr = {1, 2, 3}; c.ids[0] = -5; CHECK(c.run() == PPR_ERR_ARG); }
  { Call c; c.has_ids = false; c.w[0] = -1.0; CHECK(c.run() == PPR_ERR_ARG); }
  return 0;
}

static int test_empty() {
  // Q == 0: nothing to answer, and no output is needed; the other refusals still hold
  { Call c; c.Q = 0; c.qptr = {0}; c.outs_ok = false; c.has_ids = false; c.has_w = false; CHECK(c.run() == PPR_OK); }
  { Call c; c.Q = 0; c.qptr = {0}; c.Kq = 0; CHECK(c.run() == PPR_ERR_K); }
  { Call c; c.Q = 0; c.qptr = {3}; CHECK(c.run() == PPR_ERR_ARG); }
  // empty queries: no ids pointer needed when there is no id at all; an empty query beside a full one
  { Call c; c.Q = 3; c.qptr = {0, 0, 0, 0}; c.has_ids = false; c.has_w = false; CHECK(c.run() == PPR_OK); }
  {
    Call c;
    c.Q = 3;
    c.qptr = {0, 0, 3, 3};
    c.w = {0.0, 0.0, 0.0};
    CHECK(c.run() == PPR_ERR_ARG);
    c.w = {1.0, 1.0, 2.0};
    CHECK(c.run() == PPR_OK);
    CHECK(c.fac.size() == 3 && c.fac[0] == 0.25 && c.fac[1] == 0.25 && c.fac[2] == 0.5);
  }
  return 0;
}

static int test_factors() {
  // no weights: 1 / count
  {
    Call c;
    c.has_w = false;
    CHECK(c.run() == PPR_OK);
    CHECK(c.fac.size() == 3);
    CHECK(same_bits(c.fac[0], 1.0 / 2.0) && same_bits(c.fac[1], 1.0 / 2.0) && same_bits(c.fac[2], 1.0));
  }
  {
    Call c;
    c.Q = 1;
    c.qptr = {0, 3};
    c.ids = {0, 1, 2};
    c.has_w = false;
    CHECK(c.run() == PPR_OK);
    for (int i = 0; i < 3; i++) CHECK(same_bits(c.fac[(size_t)i], 1.0 / 3.0));
  }
  // W is summed left to right: (1e16 + 1) + 1 = 1e16 (each 1 is half an ulp and rounds to even),
  // 1 + 1 + 1e16 would be 1e16 + 2
  {
    Call c;
    c.Q = 1;
    c.qptr = {0, 3};
    c.ids = {0, 1, 2};
    c.w = {1e16, 1.0, 1.0};
    CHECK(c.run() == PPR_OK);
    volatile double W = 0.0;
    W = W + 1e16;
    W = W + 1.0;
    W = W + 1.0;
    volatile double Wrev = 0.0;
    Wrev = Wrev + 1.0;
    Wrev = Wrev + 1.0;
    Wrev = Wrev + 1e16;
    CHECK(W != Wrev);  // the set does tell the orders apart
    CHECK(same_bits(W, 1e16));
    CHECK(same_bits(c.fac[0], 1e16 / W) && same_bits(c.fac[1], 1.0 / W) && same_bits(c.fac[2], 1.0 / W));
    CHECK(!same_bits(c.fac[1], 1.0 / Wrev));
  }
  // per query: the second query's sum starts from 0 again
  {
    Call c;
    CHECK(c.run() == PPR_OK);
    CHECK(same_bits(c.fac[0], 1.0 / 4.0) && same_bits(c.fac[1], 3.0 / 4.0) && same_bits(c.fac[2], 5.0 / 5.0));
  }
  // a stale vector is replaced
  {
    Call c;
    c.fac.assign(100, 7.0);
    CHECK(c.run() == PPR_OK);
    CHECK(c.fac.size() == 3);
  }
  return 0;
}

static int test_rules() {
  const int sa[6] = {0, 1, 1, 0, 0, 1}, sb[6] = {0, 0, 1, 1, 0, 0};
  for (int it = 0; it < 6; it++) {
    const SlotPair s = slot_pair(it);
    CHECK(s.sA == sa[it] && s.sB == sb[it]);
  }
  CHECK(pow2_at_least_k(1) == 1);
  CHECK(pow2_at_least_k(2) == 2);
  CHECK(pow2_at_least_k(3) == 4);
  CHECK(pow2_at_least_k(4096) == 4096);
  CHECK(pow2_at_least_k(4095) == 4096);
  CHECK(pow2_at_least_k(5) == 8);
  const int32_t ids[3] = {0, 4, 9};
  CHECK(check_ids(ids, 3, 10) == PPR_OK);
  CHECK(check_ids(ids, 3, 9) == PPR_ERR_SOURCE);
  CHECK(check_ids(ids, 2, 9) == PPR_OK);
  CHECK(check_ids(nullptr, 0, 9) == PPR_OK);
  // hash32: values of the host copy this header replaced (rquery.hip's h_hash32), computed before it went
  CHECK(pprd::hash32(0x00000000u) == 0x00000000u);
  CHECK(pprd::hash32(0x00000001u) == 0x688990c0u);
  CHECK(pprd::hash32(0x00003039u) == 0x912efcf7u);
  CHECK(pprd::hash32(0x7fffffffu) == 0x8d29ffb8u);
  CHECK(pprd::hash32(0xffffffffu) == 0x6768824au);
  CHECK(pprd::hash32(0x9e3779b9u) == 0x01fce552u);
  return 0;
}

int main() {
  if (test_refusals() || test_empty() || test_factors() || test_rules()) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
