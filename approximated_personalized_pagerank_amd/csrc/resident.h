// resident.h -- device helpers of the kernels that read a plan's resident baskets (query.h,
// rquery.h, propagate.h): where a node's current row is and how long, what key stands behind a
// stored id, the read-only probe of a grouped key table, and the tail every top-Kq answer shares:
// select, compact, sort, write the padded result row.
#pragma once
#include "xs_table.h"

namespace pprk {

// slot of node u's current row (sA / sB: resident_args.h slot_pair)
__device__ __forceinline__ int res_slot(const uint8_t* part, int sA, int sB, int64_t u) { return part[u] ? sB : sA; }
// its length, clamped to what a row can hold: every row index derived from it stays in bounds
__device__ __forceinline__ int res_len(const DevSlab& s, int slot, int64_t u) {
  const int len = s.len[s.lrow(slot, u)];
  return len < 0 ? 0 : len > s.L ? s.L : len;
}
// stored id -> key, -1 for an id no key in [0, n) stands behind. HK = the rows may hold hot-tagged
// ids (they do after a chain-mode run); the hot set's keys are node ids below n (merge_hot.h
// k_hot_collect walks k < n), so the check of a decoded key never fires on a sound slab. n < 2^31
// (plan creation refuses more), so one unsigned 32-bit compare is both bounds -- a 64-bit compare per
// candidate cost the wave-tier query kernel 1 %. A caller that tests `(uint32_t)key >= (uint32_t)s.n`
// instead of `key < 0` repeats that very compare (-1 fails it too) and the compiler keeps one.
template <bool HK>
__device__ __forceinline__ int res_key(const DevSlab& s, int32_t id) {
  int k = id;  // (a cold id is its key; a hot-tagged one is negative)
  if (HK && id < 0) {
    const uint32_t h = (uint32_t)id & 0x7fffffffu;
    k = (int)h < s.hn ? s.hkeys[h] : -1;
  }
  return (uint32_t)k < (uint32_t)s.n ? k : -1;
}

// Slot of `key` in a key array of mask + 1 slots laid out as XTable's (key + 1, 0 = empty, probed
// in aligned groups of four), or -1. Read-only: slots are never freed and the table is never full,
// so a group with an empty slot and no match ends the search.
__device__ __forceinline__ int res_find(const uint32_t* keys, uint32_t mask, int key) {
  const uint32_t tag = (uint32_t)key + 1u;
  uint32_t g = hash32((uint32_t)key) & mask & ~3u;
  for (uint32_t mv = 0; mv < ((mask + 1u) >> 2); mv++) {
    const uint4 q = *reinterpret_cast<const uint4*>(keys + g);
    const int m = xt_match(q, g, tag);
    if (m >= 0) return m;
    if (q.x == 0u || q.y == 0u || q.z == 0u || q.w == 0u) return -1;
    g = (g + 4u) & mask;
  }
  return -1;
}

// One wave: the min(n, Kq) best of the entries (keyat(i), valat(i)), i < n, by (score desc, id asc),
// handed to emit(pos, key, score bits) at consecutive positions, in list order. Returns how many.
template <class KeyAt, class ValAt, class Emit>
__device__ __forceinline__ int wave_select_compact(int n, int Kq, KeyAt keyat, ValAt valat, uint32_t* hist, Emit emit) {
  if (n <= Kq) {
    for (int i = lane_id(); i < n; i += WAVE) emit(i, keyat(i), dbits(valat(i)));
    return n;
  }
  const SelCrit c = select_top(n, Kq, keyat, valat, hist, 0u, TieIdAsc{});
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += WAVE) {
    const int i = i0 + lane_id();
    bool sel = false;
    uint64_t vb = 0;
    int key = 0;
    if (i < n) { key = keyat(i); vb = dbits(valat(i)); sel = sel_test(c, vb, TieIdAsc{}(key, 0u)); }
    const uint64_t m = __ballot(sel);
    const int pos = base + __popcll(m & lanemask_lt());
    if (sel && pos < Kq) emit(pos, key, vb);
    base += __popcll(m);
  }
  return base < Kq ? base : Kq;
}

// One wave: result row q from cnt entries in rv / rk (LDS, room for the next power of two >= cnt,
// at most cap): sorted (score desc, id asc), unused slots id -1 / score 0, the length.
__device__ __forceinline__ void write_result_row(int32_t* out_ids, double* out_sc, int32_t* out_len, int64_t q, int Kq,
                                                 uint64_t* rv, int* rk, int cnt, int cap) {
  row_sort(rv, rk, cnt, cap);
  const int64_t o = q * (int64_t)Kq;
  for (int i = lane_id(); i < Kq; i += WAVE) {
    out_ids[o + i] = i < cnt ? rk[i] : -1;
    out_sc[o + i] = i < cnt ? bitsd(rv[i]) : 0.0;
  }
  if (lane_id() == 0) out_len[q] = cnt;
}

}  // namespace pprk
