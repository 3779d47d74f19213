// sweep.h -- device code of the sweep-cut local clustering (ppr_grank_plan_sweep,
// ppr_grank_plan_sweep_vectors; sweep.hip; host planning and the shared rules: sweep_plan.h).
//
// A source's row (its current basket, or a caller's sparse vector) is ordered by
// r = fl(score / max(deg, 1)) descending, key ascending (Andersen, Chung & Lang), cut at max_size
// entries and at the volume cap; the `swept` members that remain get the ranks 0 .. swept - 1. The
// profile of the prefixes needs, for every j, the edges with both endpoints among the first j
// members: an edge a -> b between members is internal to exactly the prefixes j > max(rank a,
// rank b), so one integer histogram over max(rank a, rank b), filled by a walk over the members'
// adjacency lists, and its prefix sum give every internal_j. Integer atomics only: the histogram
// does not depend on the order of the adds, so every tier computes the same bits.
//
//   k_s_plan    one wave per row: decode, r, row_sort on r's bit pattern (r >= +0: bits order like
//               values), scan of the degrees, the stops; writes the ordered keys, the inclusive
//               volumes, swept, the walk size W = vol_swept and the tier verdict
//   k_s_wave    one wave per source, four per block, a 256-slot key -> rank table each
//   k_s_wg      one workgroup per source (one launch per table size): every wave numbers the edges
//               of a window of 64 members and takes every 4th group of 64 edges
//   k_s_slice   one workgroup per (source, edge slice): the same walk clipped to the slice, LDS bins
//               added to a 64-bit global histogram
//   k_s_final   one wave per sliced source: prefix sums, the exact argmin, the result row (the wave
//               and workgroup tiers run the same s_finish in place on their LDS bins)
#pragma once
#include "resident.h"
#include "sweep_plan.h"

namespace pprk {

constexpr int S_WPB = 4;            // waves per k_s_wave block (and per k_s_plan block of narrow rows)
constexpr int S_WG_THREADS = 256;   // k_s_wg / k_s_slice

struct SArgs {
  // the rows: resident (src, or src_base + q when null) or the caller's vectors
  const int32_t* src;
  int64_t src_base;
  const uint8_t* part;
  int sA, sB;
  const int32_t* vids;    // [nq][width_in]
  const double* vsc;
  const int32_t* vlen;    // [nq]
  int width_in;
  // the graph
  const int64_t* rp;
  const int32_t* colx;    // bit 31: the partition bit
  int64_t n, m;
  // the call
  int width;              // entries kept at most = row stride of order / volp / prof_cut
  int min_size;
  int64_t max_vol;
  // per source of the chunk
  int32_t* order;         // [nq][width] swept members in order, then -1
  int64_t* volp;          // [nq][width] vol_j at j - 1, then -1 (the volume profile)
  int32_t* swept;
  int64_t* W;
  int32_t* code;
  int32_t* rlen;          // decodable row entries
  int32_t* size;
  int64_t* cut;
  int64_t* vol;
  double* phi;
  int64_t* prof_cut;      // [nq][width] or null
};

struct STable {           // key -> rank: keys in XTable's layout, a rank beside every key, the bins
  uint32_t* keys;
  uint16_t* rank;
  uint32_t* hist;
  uint32_t mask;
};
__host__ __device__ constexpr int s_bins(int T) { return T < pprsweep::SW_MAX_WIDTH ? T : pprsweep::SW_MAX_WIDTH; }
__host__ __device__ constexpr size_t s_lds(int T) { return (size_t)T * 6 + (size_t)s_bins(T) * 4; }
__host__ __device__ constexpr size_t s_plan_lds(int Lp) { return (size_t)Lp * 12; }
__device__ __forceinline__ STable s_carve(unsigned char* p, int T) {
  STable t;
  t.keys = reinterpret_cast<uint32_t*>(p);
  t.rank = reinterpret_cast<uint16_t*>(p + (size_t)T * 4);
  t.hist = reinterpret_cast<uint32_t*>(p + (size_t)T * 6);
  t.mask = (uint32_t)T - 1u;
  return t;
}

// inclusive wave scan of 64-bit values; every lane active
__device__ __forceinline__ long long s_scan64(long long x) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const long long y = __shfl_up(x, o);
    if (lane_id() >= o) x += y;
  }
  return x;
}

// ---------------------------------------------------------------------------------------------
template <bool VEC, bool HK>
__global__ void __launch_bounds__(S_WPB * WAVE) k_s_plan(DevSlab s, SArgs a, int64_t nq, int Lp, int64_t wave_max,
                                                          int64_t wg_max) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int wv = threadIdx.x >> 6, l = lane_id();
  const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (q >= nq) return;
  unsigned char* base = smem + (size_t)wv * s_plan_lds(Lp);
  uint64_t* rv = reinterpret_cast<uint64_t*>(base);
  int* rk = reinterpret_cast<int*>(base + (size_t)Lp * 8);
  int len;
  int64_t r0;
  if (VEC) {
    len = a.vlen[q];
    len = len < 0 ? 0 : len > a.width_in ? a.width_in : len;
    r0 = q * (int64_t)a.width_in;
  } else {
    const int64_t u = a.src ? (int64_t)a.src[q] : a.src_base + q;
    const int slot = res_slot(a.part, a.sA, a.sB, u);
    len = res_len(s, slot, u);
    r0 = s.row(slot, u);
  }
  if (len > Lp) len = Lp;  // (the host sizes Lp to the row width)
  // ---- decode, r, compact (undecodable ids are skipped)
  int cnt = 0;
  for (int i0 = 0; i0 < len; i0 += WAVE) {
    const int i = i0 + l;
    bool ok = false;
    int key = -1;
    uint64_t rb = 0;
    if (i < len) {
      const int32_t id = VEC ? a.vids[r0 + i] : s.ids[r0 + i];
      key = VEC ? ((uint32_t)id < (uint32_t)a.n ? id : -1) : res_key<HK>(s, id);
      if (key >= 0) {
        const double sc = VEC ? a.vsc[r0 + i] : s.sc[r0 + i];
        int64_t d = a.rp[key + 1] - a.rp[key];
        if (d < 1) d = 1;
        rb = dbits(sc / (double)d) & 0x7fffffffffffffffull;  // (-0 orders as +0)
        ok = true;
      }
    }
    const uint64_t mk = __ballot(ok);
    if (ok) {
      const int pos = cnt + __popcll(mk & lanemask_lt());
      rv[pos] = rb;
      rk[pos] = key;
    }
    cnt += __popcll(mk);
  }
  wave_fence();
  row_sort(rv, rk, cnt, Lp);
  // ---- the stops: max_size, then the volume cap
  const int keep = cnt < a.width ? cnt : a.width;
  const int64_t o = q * (int64_t)a.width;
  int swept = 0;
  long long vol = 0;
  bool stopped = false;
  for (int i0 = 0; i0 < keep && !stopped; i0 += WAVE) {
    const int i = i0 + l;
    long long d = 0;
    int key = -1;
    if (i < keep) {
      key = rk[i];
      d = a.rp[key + 1] - a.rp[key];
      if (d < 0) d = 0;
      if (d > a.max_vol) d = a.max_vol + 1;  // (it ends the sweep either way: no sum can overflow)
    }
    const long long inc = s_scan64(d) + vol;
    const uint64_t over = __ballot(i < keep && inc > a.max_vol);
    const int here = keep - i0 < WAVE ? keep - i0 : WAVE;
    const int nok = over ? __ffsll((unsigned long long)over) - 1 : here;
    if (l < nok) {
      a.order[o + i] = key;
      a.volp[o + i] = inc;
    }
    if (nok > 0) vol = __shfl(inc, nok - 1);
    swept += nok;
    stopped = over != 0ull;
  }
  for (int i = swept + l; i < a.width; i += WAVE) {
    a.order[o + i] = -1;
    a.volp[o + i] = -1;
  }
  if (l == 0) {
    a.swept[q] = swept;
    a.W[q] = vol;
    a.rlen[q] = cnt;
    a.code[q] = pprsweep::sw_tier(vol, swept, wave_max, wg_max);
  }
}

// ---- the key -> rank table of one source, cleared and filled by nthr threads (no barrier inside)
__device__ __forceinline__ void s_clear(const STable& t, int T, int tid, int nthr) {
  for (int i = tid; i < T; i += nthr) t.keys[i] = 0u;
  for (int i = tid; i < s_bins(T); i += nthr) t.hist[i] = 0u;
}
__device__ __forceinline__ bool s_fill(const STable& t, const int32_t* ord, int swept, int tid, int nthr) {
  bool bad = false;
  XTable xt;
  xt.keys = t.keys;
  xt.lo = nullptr;
  xt.hi = nullptr;
  xt.mask = t.mask;
  for (int i = tid; i < swept; i += nthr) {
    bool ins;
    const int sl = xt_slot(xt, ord[i], ins);
    if (sl < 0) bad = true;
    else t.rank[sl] = (uint16_t)i;
  }
  return bad;
}

// The walk. Windows of 64 members: lane l holds member w0 + l's first edge and its edge count (SLICE:
// clipped to the edges [e0, e1) of the source's concatenated lists, which volp numbers), a DPP scan
// numbers the window's edges, and every lane finds the member of its edge by the binary search over
// the scan (shuffles), so that consecutive lanes read consecutive words of an adjacency list. Wave
// wv of nw takes every nw-th group of 64 edges. Per edge one probe and, on a hit, one integer add.
template <bool SLICE>
__device__ __forceinline__ void s_walk(const SArgs& a, const STable& t, const int32_t* ord, const int64_t* volp,
                                       int swept, int64_t e0, int64_t e1, int wv, int nw) {
  const int l = lane_id();
  for (int w0 = 0; w0 < swept; w0 += WAVE) {
    const int i = w0 + l;
    int n = 0;
    int64_t start = 0;
    if (i < swept) {
      const int key = ord[i];
      const int64_t b = a.rp[key], deg = a.rp[key + 1] - b;
      if (SLICE) {
        const int64_t pb = volp[i] - deg;
        const int64_t lo = pb > e0 ? pb : e0, hi = pb + deg < e1 ? pb + deg : e1;
        n = hi > lo ? (int)(hi - lo) : 0;
        start = b + (lo - pb);
      } else {
        n = deg > 0 ? (int)deg : 0;
        start = b;
      }
    }
    const int incl = wave_incl_scan(n);
    const int total = __builtin_amdgcn_readlane(incl, WAVE - 1);
    for (int c0 = wv * WAVE; c0 < total; c0 += nw * WAVE) {
      const int c = c0 + l;
      int tl = 0;  // lanes whose scan is <= c: the first lane past them owns edge c
#pragma unroll
      for (int st = 32; st; st >>= 1) {
        const int v = __shfl(incl, tl + st - 1);
        tl += v <= c ? st : 0;
      }
      const int ex = __shfl(incl - n, tl);
      const long long st0 = __shfl((long long)start, tl);
      if (c < total) {
        const int ra = w0 + tl;
        const int b = a.colx[(int64_t)st0 + (c - ex)] & 0x7fffffff;
        const int m = res_find(t.keys, t.mask, b);
        if (m >= 0) {
          const int rb = (int)t.rank[m];
          atomicAdd(&t.hist[ra > rb ? ra : rb], 1u);
        }
      }
    }
  }
}

// One wave: the profile of source q from its bins hist(i) = edges whose larger rank is i, the best
// admissible prefix by exact comparison (ties to the smaller j) and the result row.
template <class HistAt>
__device__ __forceinline__ void s_finish(const SArgs& a, int64_t q, int swept, HistAt hist) {
  const int l = lane_id();
  const int64_t o = q * (int64_t)a.width;
  long long base = 0, bc = 0, bd = 0, bv = 0;
  int bj = 0;  // 0: none yet
  for (int i0 = 0; i0 < swept; i0 += WAVE) {
    const int i = i0 + l;
    const long long h = i < swept ? (long long)hist(i) : 0;
    const long long in = s_scan64(h) + base;
    base = __shfl(in, WAVE - 1);
    if (i < swept) {
      const long long vol = a.volp[o + i], cut = vol - in;
      const long long den = vol < a.m - vol ? vol : a.m - vol;
      if (a.prof_cut) a.prof_cut[o + i] = cut;
      if (i + 1 >= a.min_size && den > 0 && (bj == 0 || pprsweep::frac_less(cut, den, bc, bd))) {
        bc = cut; bd = den; bv = vol; bj = i + 1;
      }
    }
  }
  if (a.prof_cut)
    for (int i = swept + l; i < a.width; i += WAVE) a.prof_cut[o + i] = -1;
#pragma unroll
  for (int x = 32; x; x >>= 1) {
    const long long oc = __shfl_xor(bc, x), od = __shfl_xor(bd, x), ov = __shfl_xor(bv, x);
    const int oj = __shfl_xor(bj, x);
    bool take = false;
    if (oj != 0) {
      if (bj == 0) take = true;
      else if (pprsweep::frac_less(oc, od, bc, bd)) take = true;
      else if (!pprsweep::frac_less(bc, bd, oc, od) && oj < bj) take = true;
    }
    if (take) { bc = oc; bd = od; bv = ov; bj = oj; }
  }
  if (l == 0) {
    a.size[q] = bj;
    a.cut[q] = bj ? bc : 0;
    a.vol[q] = bj ? bv : 0;
    a.phi[q] = bj ? (double)bc / (double)bd : __longlong_as_double(0x7ff0000000000000ll);
  }
}

// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(S_WPB * WAVE) k_s_wave(SArgs a, const int32_t* list, int64_t count) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int T = pprsweep::SW_WAVE_T;
  const int wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * S_WPB + wv;
  if (w >= count) return;
  const STable t = s_carve(smem + (size_t)wv * s_lds(T), T);
  const int64_t q = list[w];
  int swept = a.swept[q];
  if (swept > 3 * T / 4) { swept = 0; if (lane_id() == 0) probe_fail(); }  // (cannot happen: sw_tier)
  const int32_t* ord = a.order + q * (int64_t)a.width;
  s_clear(t, T, lane_id(), WAVE);
  wave_fence();
  const bool bad = s_fill(t, ord, swept, lane_id(), WAVE);
  wave_fence();
  if (__ballot(bad) && lane_id() == 0) probe_fail();
  s_walk<false>(a, t, ord, nullptr, swept, 0, 0, 0, 1);
  wave_fence();
  s_finish(a, q, swept, [&](int i) { return t.hist[i]; });
}

// the workgroup's table of one source; returns swept (0 and the error word when it cannot fit)
__device__ __forceinline__ int s_wg_table(const SArgs& a, const STable& t, int T, int64_t q, const int32_t* ord) {
  int swept = a.swept[q];
  if (4 * swept > 3 * T || swept > s_bins(T)) { swept = 0; if (threadIdx.x == 0) probe_fail(); }  // (cannot happen)
  s_clear(t, T, threadIdx.x, blockDim.x);
  __syncthreads();
  const bool bad = s_fill(t, ord, swept, threadIdx.x, blockDim.x);
  if (__ballot(bad) && lane_id() == 0) probe_fail();
  __syncthreads();
  return swept;
}

__global__ void __launch_bounds__(S_WG_THREADS) k_s_wg(SArgs a, const int32_t* list, int T) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int64_t q = list[blockIdx.x];
  const STable t = s_carve(smem, T);
  const int32_t* ord = a.order + q * (int64_t)a.width;
  const int swept = s_wg_table(a, t, T, q, ord);
  s_walk<false>(a, t, ord, nullptr, swept, 0, 0, threadIdx.x >> 6, blockDim.x >> 6);
  __syncthreads();
  if (threadIdx.x >= WAVE) return;
  s_finish(a, q, swept, [&](int i) { return t.hist[i]; });
}

__global__ void __launch_bounds__(S_WG_THREADS) k_s_slice(SArgs a, const pprsweep::STask* tasks,
                                                          unsigned long long* gh) {
  extern __shared__ __align__(16) unsigned char smem[];
  const pprsweep::STask tk = tasks[blockIdx.x];
  const int64_t q = tk.q;
  const int T = pprsweep::sw_table_slots(a.swept[q]);
  const STable t = s_carve(smem, T);
  const int32_t* ord = a.order + q * (int64_t)a.width;
  const int swept = s_wg_table(a, t, T, q, ord);
  s_walk<true>(a, t, ord, a.volp + q * (int64_t)a.width, swept, tk.e0, tk.e1, threadIdx.x >> 6, blockDim.x >> 6);
  __syncthreads();
  unsigned long long* row = gh + (int64_t)tk.row * a.width;
  for (int i = threadIdx.x; i < swept; i += blockDim.x) {
    const uint32_t h = t.hist[i];
    if (h) atomicAdd(&row[i], (unsigned long long)h);
  }
}

__global__ void __launch_bounds__(WAVE) k_s_final(SArgs a, const int32_t* list, const unsigned long long* gh) {
  const int64_t q = list[blockIdx.x];
  const unsigned long long* row = gh + (int64_t)blockIdx.x * a.width;
  s_finish(a, q, a.swept[q], [&](int i) { return row[i]; });
}

}  // namespace pprk
