// xs_table.h -- the exact-sum primitives shared by the GRank merge (merge_xs.h) and the
// preference-set queries (query.h): the 96-bit fixed-point conversion of one contribution and the
// LDS table that adds such contributions per key with atomics.
#pragma once
#include "ppr_common.h"

namespace pprk {

// floor(p * 2^F) of p in [0, 2^(95 - F)): lo = low 64 bits, hi = bits 64..94 (F = 93: p < 4)
__device__ __forceinline__ void xs_conv(double p, unsigned long long& lo, uint32_t& hi, int F = XS_F) {
  const unsigned long long b = dbits(p);
  int e = (int)((b >> 52) & 0x7ffu);
  unsigned long long m = b & ((1ull << 52) - 1ull);
  if (e) m |= 1ull << 52; else e = 1;
  const int sh = e - 1075 + F;
  if (sh >= 0) {
    lo = m << sh;
    hi = sh > 11 ? (uint32_t)(m >> (64 - sh)) : 0u;
  } else {
    lo = -sh < 64 ? (m >> -sh) : 0ull;
    hi = 0u;
  }
}

// X * 2^-93 rounded to nearest even: the top 64 bits of X with a sticky bit, one correctly rounded
// u64 -> f64 conversion, an exact power-of-two scale (oracle_xs_to_double)
__device__ __forceinline__ double xs_to_double(uint32_t hi, unsigned long long lo, int F = XS_F) {
  if (hi == 0u) return ldexp((double)lo, -F);
  const int n = 32 - __clz(hi);
  const unsigned long long top = ((unsigned long long)hi << (64 - n)) | (lo >> n);
  const unsigned long long sticky = (lo & ((1ull << n) - 1ull)) != 0ull ? 1ull : 0ull;
  return ldexp((double)(top | sticky), n - F);
}

// value of a single contribution p as the exact path stores it: a lower bound of the total of any
// key that receives p (totals of nonnegative terms only grow, rounding is monotone)
__device__ __forceinline__ double xs_single(double p, int F = XS_F) {
  unsigned long long lo;
  uint32_t hi;
  xs_conv(p, lo, hi, F);
  return xs_to_double(hi, lo, F);
}

// LDS table of 16-B slots in three arrays: keys u32 (key + 1, 0 = empty), lo u64 (low word of the
// sum), hi u32 (high word). Slots are probed in aligned groups of four keys, one ds_read_b128 per
// step: the longest probe among a group's 64 lanes (the wave waits for it) stays short at fills
// where single-slot linear probing ran long chains.
struct XTable {
  uint32_t* keys;
  unsigned long long* lo;
  uint32_t* hi;
  uint32_t mask;
};

// find-or-insert `key`, then add X: the low word's returning add yields its carry, which goes
// with the high word into hi. Returns 1 when this lane inserted the key, 0 when it was there, -1
// when the probe ran out (T/4 groups visited or T/4 insert races lost: the table is full) -- no
// add then, and the caller takes its overflow path. Every caller sizes or budgets its table so
// that this cannot happen; the bound turns a sizing bug into a redone source instead of a hang
// (tests: PPR_WAVE_TDIV, PPR_XR_BUDGET=over force it).
__device__ __forceinline__ int xt_add(const XTable& t, int key, unsigned long long xlo, uint32_t xhi) {
  const uint32_t tag = (uint32_t)key + 1u;
  uint32_t g = hash32((uint32_t)key) & t.mask & ~3u;
  int ins = 0;
  uint32_t h = 0;
  const uint32_t groups = (t.mask + 1u) >> 2;
  uint32_t moves = 0, races = 0;
  for (;;) {
    if (moves >= groups || races > groups) return -1;
    const uint4 q = *reinterpret_cast<const uint4*>(t.keys + g);
    if (q.x == tag) { h = g; break; }
    if (q.y == tag) { h = g + 1; break; }
    if (q.z == tag) { h = g + 2; break; }
    if (q.w == tag) { h = g + 3; break; }
    const int e = q.x == 0u ? 0 : q.y == 0u ? 1 : q.z == 0u ? 2 : q.w == 0u ? 3 : -1;
    if (e >= 0) {
      const uint32_t prev = atomicCAS(&t.keys[g + e], 0u, tag);
      if (prev == 0u) { h = g + e; ins = 1; break; }
      if (prev == tag) { h = g + e; break; }
      races++;
      continue;  // another key took it: read the group again
    }
    g = (g + 4u) & t.mask;
    moves++;
  }
  const unsigned long long old = atomicAdd(&t.lo[h], xlo);
  const uint32_t up = xhi + ((old + xlo < old) ? 1u : 0u);
  if (up) atomicAdd(&t.hi[h], up);
  return ins;
}

// the slot of `key` within a loaded group of four (or -1)
__device__ __forceinline__ int xt_match(const uint4& q, uint32_t g, uint32_t tag) {
  return q.x == tag ? (int)g : q.y == tag ? (int)g + 1 : q.z == tag ? (int)g + 2 : q.w == tag ? (int)g + 3 : -1;
}
// find-or-insert only (xt_add's bounded probe); returns the slot, `ins` when this lane inserted,
// -1 when the table is full
__device__ __forceinline__ int xt_slot(const XTable& t, int key, bool& ins) {
  const uint32_t tag = (uint32_t)key + 1u;
  uint32_t g = hash32((uint32_t)key) & t.mask & ~3u;
  ins = false;
  const uint32_t groups = (t.mask + 1u) >> 2;
  uint32_t moves = 0, races = 0;
  while (moves < groups && races <= groups) {
    const uint4 q = *reinterpret_cast<const uint4*>(t.keys + g);
    const int m = xt_match(q, g, tag);
    if (m >= 0) return m;
    const int e = q.x == 0u ? 0 : q.y == 0u ? 1 : q.z == 0u ? 2 : q.w == 0u ? 3 : -1;
    if (e >= 0) {
      const uint32_t prev = atomicCAS(&t.keys[g + e], 0u, tag);
      if (prev == 0u) { ins = true; return (int)(g + e); }
      if (prev == tag) return (int)(g + e);
      races++;
      continue;
    }
    g = (g + 4u) & t.mask;
    moves++;
  }
  return -1;
}

__host__ __device__ constexpr size_t xt_bytes(int T) { return (size_t)T * 16; }
// carve a T-slot table at p (16-B aligned)
__device__ __forceinline__ XTable xt_carve(unsigned char* p, int T) {
  XTable t;
  t.keys = reinterpret_cast<uint32_t*>(p);
  t.lo = reinterpret_cast<unsigned long long*>(p + (size_t)T * 4);
  t.hi = reinterpret_cast<uint32_t*>(p + (size_t)T * 12);
  t.mask = (uint32_t)T - 1u;
  return t;
}

}  // namespace pprk
