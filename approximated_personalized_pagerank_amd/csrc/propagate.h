// propagate.h -- device code of the feature propagation through a plan's resident baskets
// (ppr_grank_plan_propagate / ppr_grank_plan_propagate_t, propagate.hip; semantics: include/ppr_hip.h).
//
// Forward, Z = B[S] H: a gather-bound SpMM over rows of at most L entries.
//   k_p_fwd<DT, V, HK>  a group of G = 1 << lgG lanes owns one (position, column tile); a lane owns V
//                   adjacent columns (one 4- / 8- / 16-byte load) and V fp64 accumulators. G is the
//                   power of two >= ceil(F / V), 4 .. 64, so with narrow features a wave carries
//                   64 / G positions at once: the one-entry rows of dangling sources (half of an
//                   RMAT graph) share their wave trip with 64 / G - 1 other rows instead of taking
//                   one each. The group's lanes load up to G (id, score) entries at once, one per
//                   lane, and broadcast them entry by entry; four feature rows are in flight per
//                   group before their fmas run, in stored order.
// Transposed, Y = B[S]^T G: store, then sum per destination through an inverted index.
//   k_p_walk<HK, MODE>  the batch's rows, a group of lanes per position: MODE 2 counts postings per
//                   key (integer atomics into PS_SHARDS counter arrays picked by the position, so a
//                   key that sits in most rows does not queue its adds in one channel), MODE 0 counts
//                   a position's keys inside the pass's key range, MODE 1 emits (key - k0,
//                   position << 12 | j) at the position's offset: position-major order.
//   k_p_scount / k_p_sscatter  a stable LSD radix sort by key, 8 bits per pass, in the shape of the
//                   hub pipeline's count / scatter: a wave owns a tile of PS_TILE consecutive
//                   entries, counts its digits, the (digit, tile) counts are scanned, and the wave
//                   walks its tile again in order, ranking equal digits by lane order. rocPRIM's
//                   radix_sort_pairs was not used: its onesweep kernels keep 48 bytes of scratch per
//                   lane, which build.py refuses for this library's own kernels.
//   k_p_kstart      first sorted posting of every key of the range (binary search): the run bounds
//   k_p_tsum<DT, V> one wave per (chunk task, column tile): the fp64 fma chain over the chunk's
//                   postings in order; writes the output row or an fp64 partial row
//   k_p_tfold<DT>   a key with several chunks: its partial rows added in chunk order, rounded once
//   k_p_zero<DT>    the range's keys without postings: zero rows
// No float atomics anywhere; every index is bounded (positions and keys clamped or skipped).
#pragma once
#include "prop_plan.h"
#include "resident.h"

namespace pprk {

constexpr int P_THREADS = 256;            // 4 waves per block
constexpr int P_WPB = P_THREADS / 64;
constexpr int PS_TILE = 2048;             // sort: entries per wave
constexpr int PS_SHARDS = 8;              // per-key counter arrays of the count pass
constexpr int P_JBITS = 12;               // posting value = position << 12 | j (j < MAX_L = 4096)

struct PArgs {
  const uint8_t* part;
  int sA, sB;             // current slot of a partition-0 / partition-1 node
  const int32_t* src;     // [S] sources, null: position i is source i
  int64_t S;
  int norm;               // PPR_PROP_ROW_NORMALIZE
};

__device__ __forceinline__ int p_src(const DevSlab& s, const PArgs& a, int64_t i) {
  int64_t u = a.src ? (int64_t)a.src[i] : i;  // (checked on the host; clamped all the same)
  return (int)(u < 0 ? 0 : u >= s.n ? s.n - 1 : u);
}
// (slot, length and stored id -> key: resident.h; an id no key stands behind is skipped by every kernel alike)

// ---- feature elements: DT 0 = fp32, 1 = bf16 ---------------------------------------------------
// V elements of one lane, as loaded
template <int DT, int V>
struct PRaw {
  static constexpr int ESZ = DT ? 2 : 4;
  static constexpr int BYTES = V * ESZ;
  static constexpr int NW = BYTES >= 4 ? BYTES / 4 : 1;
  uint32_t w[NW];
  __device__ __forceinline__ void load(const void* base, int64_t e) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base) + e * ESZ;
    if constexpr (BYTES == 16) {
      const uint4 x = *reinterpret_cast<const uint4*>(p);
      w[0] = x.x; w[1 % NW] = x.y; w[2 % NW] = x.z; w[3 % NW] = x.w;
    } else if constexpr (BYTES == 8) {
      const uint2 x = *reinterpret_cast<const uint2*>(p);
      w[0] = x.x; w[1 % NW] = x.y;
    } else if constexpr (BYTES == 4) {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
      w[0] = *reinterpret_cast<const uint16_t*>(p);
    }
  }
  template <int K>
  __device__ __forceinline__ double get() const {
    if constexpr (DT == 0) return (double)__uint_as_float(w[K]);
    else return (double)__uint_as_float(((w[K >> 1] >> ((K & 1) * 16)) & 0xffffu) << 16);
  }
};

// bit pattern of x rounded to nearest even in the feature type, straight from the fp64 value
// (bf16 does not pass through fp32: that would round twice)
template <int DT>
__device__ __forceinline__ uint32_t p_round(double x) {
  constexpr int MB = DT ? 7 : 23;
  const uint64_t b = dbits(x);
  const uint32_t sign = (uint32_t)(b >> 63) << (MB + 8);
  const int ex = (int)((b >> 52) & 0x7ffu);
  const uint64_t man = b & ((1ull << 52) - 1ull);
  if (ex == 0x7ff) return sign | (0xffu << MB) | (man ? 1u << (MB - 1) : 0u);
  if (ex == 0) return sign;  // zero, or an fp64 subnormal: far below half the smallest subnormal
  const int e = ex - 1023;
  if (e > 127) return sign | (0xffu << MB);
  int sh = 52 - MB;
  if (e < -126) sh += -126 - e;
  if (sh > 54) return sign;
  const uint64_t full = man | (1ull << 52);
  uint64_t q = full >> sh;
  const uint64_t rem = full & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
  if (rem > half || (rem == half && (q & 1ull))) q++;
  if (e < -126) return sign | (uint32_t)q;  // subnormal (q = 2^MB is the smallest normal's pattern)
  uint32_t r = ((uint32_t)(e + 126) << MB) + (uint32_t)q;  // q carries the implicit bit: exponent field e + 127
  if (r > (0xffu << MB)) r = 0xffu << MB;
  return sign | r;
}

template <int DT>
__device__ __forceinline__ void p_store1(void* base, int64_t e, double x) {
  const uint32_t r = p_round<DT>(x);
  if constexpr (DT == 0) reinterpret_cast<uint32_t*>(base)[e] = r;
  else reinterpret_cast<uint16_t*>(base)[e] = (uint16_t)r;
}

template <int DT, int V>
__device__ __forceinline__ void p_store(void* base, int64_t e, const double (&acc)[V]) {
  constexpr int ESZ = DT ? 2 : 4;
  unsigned char* p = reinterpret_cast<unsigned char*>(base) + e * ESZ;
  if constexpr (V == 1) {
    p_store1<DT>(base, e, acc[0]);
  } else if constexpr (DT == 0) {  // V == 4
    uint4 x;
    x.x = p_round<0>(acc[0]); x.y = p_round<0>(acc[1 % V]); x.z = p_round<0>(acc[2 % V]); x.w = p_round<0>(acc[3 % V]);
    *reinterpret_cast<uint4*>(p) = x;
  } else if constexpr (V == 4) {
    uint2 x;
    x.x = p_round<1>(acc[0]) | (p_round<1>(acc[1 % V]) << 16);
    x.y = p_round<1>(acc[2 % V]) | (p_round<1>(acc[3 % V]) << 16);
    *reinterpret_cast<uint2*>(p) = x;
  } else {  // bf16, V == 8
    uint4 x;
    x.x = p_round<1>(acc[0]) | (p_round<1>(acc[1 % V]) << 16);
    x.y = p_round<1>(acc[2 % V]) | (p_round<1>(acc[3 % V]) << 16);
    x.z = p_round<1>(acc[4 % V]) | (p_round<1>(acc[5 % V]) << 16);
    x.w = p_round<1>(acc[6 % V]) | (p_round<1>(acc[7 % V]) << 16);
    *reinterpret_cast<uint4*>(p) = x;
  }
}

template <int DT, int V, int K = 0>
__device__ __forceinline__ void p_fma(double (&acc)[V], double w, const PRaw<DT, V>& x) {
  if constexpr (K < V) {
    acc[K] = __builtin_fma(w, x.template get<K>(), acc[K]);
    p_fma<DT, V, K + 1>(acc, w, x);
  }
}

// The gather of up to G broadcast entries: `row` (a feature row index, -1 = none) and `wt` are held
// one entry per lane of the group starting at lane g0; entries [0, cnt) are consumed in order, four
// feature-row loads in flight. G is a multiple of 4, so t + q stays inside the group.
template <int DT, int V>
__device__ __forceinline__ void p_gather(double (&acc)[V], int row, double wt, int g0, int cnt, const void* X,
                                         int64_t ldx, int c, bool colok) {
  for (int t = 0; t < cnt; t += 4) {
    int rq[4];
    double wq[4];
    PRaw<DT, V> x[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      rq[q] = __shfl(row, g0 + t + q);
      wq[q] = __shfl(wt, g0 + t + q);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int k = 0; k < PRaw<DT, V>::NW; k++) x[q].w[k] = 0u;
      if (rq[q] >= 0 && colok) x[q].load(X, (int64_t)rq[q] * ldx + c);
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (rq[q] >= 0 && colok) p_fma<DT, V>(acc, wq[q], x[q]);
  }
}

// ---- forward -----------------------------------------------------------------------------------
template <int DT, int V, bool HK>
__global__ void __launch_bounds__(P_THREADS) k_p_fwd(DevSlab s, PArgs a, const void* H, int64_t ldh, void* Z,
                                                    int64_t ldz, int F, int lgG, int64_t ngrp) {
  const int l = lane_id(), G = 1 << lgG, R = WAVE >> lgG, r = l >> lgG, j = l & (G - 1), g0 = l & ~(G - 1);
  const int64_t w = (int64_t)blockIdx.x * P_WPB + (threadIdx.x >> 6);
  if (w >= ngrp) return;  // (the whole wave)
  const int64_t i = w * R + r;
  const int c = ((int)blockIdx.y * G + j) * V;
  const bool colok = c < F;  // (F is a multiple of V)
  int len = 0;
  int64_t row = 0;
  if (i < a.S) {
    const int u = p_src(s, a, i);
    const int slot = res_slot(a.part, a.sA, a.sB, u);
    len = res_len(s, slot, u);
    row = s.row(slot, u);
  }
  double W = 0.0;
  if (a.norm)  // one sequential chain in stored order (a wave reduction would change the bits)
    for (int t = 0; t < len; t++) W = W + s.sc[row + t];
  int maxlen = len;
#pragma unroll
  for (int o = 32; o; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
  double acc[V];
#pragma unroll
  for (int k = 0; k < V; k++) acc[k] = 0.0;
  for (int b = 0; b < maxlen; b += G) {
    int key = -1;
    double wt = 0.0;
    if (b + j < len) {
      key = res_key<HK>(s, s.ids[row + b + j]);
      const double sc = s.sc[row + b + j];
      wt = a.norm ? pprprop::prop_weight(sc, W) : sc;
    }
    p_gather<DT, V>(acc, key, wt, g0, min(G, maxlen - b), H, ldh, c, colok);
  }
  if (i < a.S && colok) p_store<DT, V>(Z, i * ldz + c, acc);
}

// ---- transposed: per-position lengths and row sums ---------------------------------------------
__global__ void __launch_bounds__(P_THREADS) k_p_len(DevSlab s, PArgs a, double* wpos, unsigned long long* tot) {
  const int64_t i = (int64_t)blockIdx.x * P_THREADS + threadIdx.x;
  unsigned long long len = 0ull;
  if (i < a.S) {
    const int u = p_src(s, a, i);
    const int slot = res_slot(a.part, a.sA, a.sB, u);
    const int n = res_len(s, slot, u);
    len = (unsigned long long)n;
    if (wpos) {
      const int64_t row = s.row(slot, u);
      double W = 0.0;
      for (int t = 0; t < n; t++) W = W + s.sc[row + t];
      wpos[i] = W;
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) len += __shfl_xor(len, o);
  if (lane_id() == 0 && len) atomicAdd(tot, len);
}

// MODE 0: pcnt[i] = keys of position i inside [k0, k1); MODE 1: emit them at poff[i]; MODE 2: count
// every key into its shard
template <bool HK, int MODE>
__global__ void __launch_bounds__(P_THREADS) k_p_walk(DevSlab s, PArgs a, int lgG, int64_t ngrp, int k0, int k1,
                                                     int32_t* pcnt, const int32_t* poff, uint32_t* keys,
                                                     int64_t* vals, int M, uint32_t* kc) {
  const int l = lane_id(), G = 1 << lgG, R = WAVE >> lgG, r = l >> lgG, j = l & (G - 1), g0 = l & ~(G - 1);
  const int64_t w = (int64_t)blockIdx.x * P_WPB + (threadIdx.x >> 6);
  if (w >= ngrp) return;
  const int64_t i = w * R + r;
  int len = 0;
  int64_t row = 0;
  if (i < a.S) {
    const int u = p_src(s, a, i);
    const int slot = res_slot(a.part, a.sA, a.sB, u);
    len = res_len(s, slot, u);
    row = s.row(slot, u);
  }
  int maxlen = len;
#pragma unroll
  for (int o = 32; o; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
  const uint64_t gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const int base = (MODE == 1 && i < a.S) ? poff[i] : 0;
  int tot = 0;
  for (int b = 0; b < maxlen; b += G) {
    const int e = b + j;
    int key = -1;
    if (e < len) key = res_key<HK>(s, s.ids[row + e]);
    const bool hit = key >= k0 && key < k1;
    const uint64_t gm = (__ballot(hit) >> g0) & gmask;
    if (hit) {
      if (MODE == 1) {
        const int pos = base + tot + __popcll(gm & ((1ull << j) - 1ull));
        if (pos >= 0 && pos < M) {  // (the count pass walked the same rows)
          keys[pos] = (uint32_t)(key - k0);
          vals[pos] = (i << P_JBITS) | (int64_t)e;
        }
      }
      if (MODE == 2) atomicAdd(&kc[(int64_t)(i & (PS_SHARDS - 1)) * s.n + key], 1u);
    }
    tot += __popcll(gm);
  }
  if (MODE == 0 && j == 0 && i < a.S) pcnt[i] = tot;
}

// per-key counts: the shards summed (a key has at most S postings; clamped to int32)
__global__ void __launch_bounds__(P_THREADS) k_p_kfold(const uint32_t* kc, int64_t n, int32_t* cnt) {
  const int64_t k = (int64_t)blockIdx.x * P_THREADS + threadIdx.x;
  if (k >= n) return;
  unsigned long long c = 0ull;
  for (int sh = 0; sh < PS_SHARDS; sh++) c += kc[(int64_t)sh * n + k];
  cnt[k] = (int32_t)(c > 0x7fffffffull ? 0x7fffffffull : c);
}

// ---- the stable sort: one 8-bit digit per pass -------------------------------------------------
__global__ void __launch_bounds__(P_THREADS) k_p_scount(const uint32_t* keys, int M, int shift, int32_t* hist,
                                                       int ntiles) {
  __shared__ int32_t h[P_WPB][256];
  const int wv = threadIdx.x >> 6, l = lane_id();
  const int tile = (int)blockIdx.x * P_WPB + wv;
  if (tile >= ntiles) return;
  for (int d = l; d < 256; d += WAVE) h[wv][d] = 0;
  wave_fence();
  const int b0 = tile * PS_TILE, e0 = min(M, b0 + PS_TILE);
  for (int t = b0 + l; t < e0; t += WAVE) atomicAdd(&h[wv][(keys[t] >> shift) & 255u], 1);
  wave_fence();
  for (int d = l; d < 256; d += WAVE) hist[(int64_t)d * ntiles + tile] = h[wv][d];
}

// offs = the exclusive scan of hist in (digit, tile) order: where the tile's first entry of each
// digit goes. Equal digits of a tile keep their order: a lane's rank among the lanes of its step
// with the same digit is its place among them, and the steps run in order.
__global__ void __launch_bounds__(P_THREADS) k_p_sscatter(const uint32_t* kin, const int64_t* vin, uint32_t* kout,
                                                         int64_t* vout, int M, int shift, const int32_t* offs,
                                                         int ntiles) {
  __shared__ int32_t base[P_WPB][256];
  const int wv = threadIdx.x >> 6, l = lane_id();
  const int tile = (int)blockIdx.x * P_WPB + wv;
  if (tile >= ntiles) return;
  for (int d = l; d < 256; d += WAVE) base[wv][d] = offs[(int64_t)d * ntiles + tile];
  wave_fence();
  const int b0 = tile * PS_TILE, e0 = min(M, b0 + PS_TILE);
  for (int t0 = b0; t0 < e0; t0 += WAVE) {
    const int t = t0 + l;
    const bool valid = t < e0;
    const uint32_t key = valid ? kin[t] : 0u;
    const int64_t val = valid ? vin[t] : 0;
    const uint32_t d = (key >> shift) & 255u;
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const bool on = (d >> bit) & 1u;
      const uint64_t bal = __ballot(on);
      m &= on ? bal : ~bal;
    }
    if (valid) {
      const int pos = base[wv][d] + __popcll(m & lanemask_lt());
      if (pos >= 0 && pos < M) { kout[pos] = key; vout[pos] = val; }
    }
    wave_fence();
    if (valid && (m >> l) == 1ull) base[wv][d] += __popcll(m);  // the last lane of each digit's set
    wave_fence();
  }
}

// kstart[t] = first sorted posting with key >= t, t = 0 .. nk
__global__ void __launch_bounds__(P_THREADS) k_p_kstart(const uint32_t* keys, int M, int64_t nk, int32_t* kstart) {
  const int64_t t = (int64_t)blockIdx.x * P_THREADS + threadIdx.x;
  if (t > nk) return;
  int lo = 0, hi = M;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)keys[mid] < t) lo = mid + 1; else hi = mid;
  }
  kstart[t] = lo;
}

// ---- the chunk tasks, planned on the device (pprprop::build_chunk_tasks's rule, key by key) -----
// what key k0 + k needs: chunk tasks, partial rows, fold tasks; entry nk is 0, so the exclusive scans
// of the three arrays end in the totals
__global__ void __launch_bounds__(P_THREADS) k_p_tcount(const int32_t* kstart, int64_t nk, int32_t* nt, int32_t* np,
                                                       int32_t* nf) {
  const int64_t k = (int64_t)blockIdx.x * P_THREADS + threadIdx.x;
  if (k > nk) return;
  int m = 0;
  if (k < nk) {
    const int c = kstart[k + 1] - kstart[k];
    m = c > 0 ? (c + pprprop::PROP_CHUNK - 1) / pprprop::PROP_CHUNK : 0;
  }
  nt[k] = m;
  np[k] = m > 1 ? m : 0;
  nf[k] = m > 1 ? 1 : 0;
}

// tasks of a key at toff[k], in chunk order; its partial rows poff[k] ..; its fold task at foff[k]
__global__ void __launch_bounds__(P_THREADS) k_p_tplan(const int32_t* kstart, int64_t nk, int64_t k0, const int32_t* toff,
                                                      const int32_t* poff, const int32_t* foff, pprprop::PTask* tasks,
                                                      int64_t ntask, pprprop::PFold* folds, int64_t nfold) {
  const int64_t k = (int64_t)blockIdx.x * P_THREADS + threadIdx.x;
  if (k >= nk) return;
  const int b = kstart[k], e = kstart[k + 1];
  if (e <= b) return;
  const int m = (e - b + pprprop::PROP_CHUNK - 1) / pprprop::PROP_CHUNK;
  for (int c = 0; c < m; c++) {
    const int64_t t = (int64_t)toff[k] + c;
    const int o = b + c * pprprop::PROP_CHUNK;
    if (t >= 0 && t < ntask)
      tasks[t] = pprprop::PTask{(int64_t)o, m > 1 ? (int64_t)poff[k] + c : (int64_t)-1, (int32_t)(k0 + k),
                                min(pprprop::PROP_CHUNK, e - o)};
  }
  if (m > 1 && foff[k] >= 0 && (int64_t)foff[k] < nfold) folds[foff[k]] = pprprop::PFold{(int64_t)poff[k], (int32_t)(k0 + k), m};
}

// ---- transposed sums ---------------------------------------------------------------------------
// columns [c0, c1) of the call (one column block); partial rows are c1 - c0 <= ldp wide
template <int DT, int V>
__global__ void __launch_bounds__(P_THREADS) k_p_tsum(DevSlab s, PArgs a, const double* wpos, const pprprop::PTask* tasks,
                                                     int64_t ntask, const int64_t* vals, int M, const void* Gm,
                                                     int64_t ldg, void* Y, int64_t ldy, double* parts, int64_t nparts,
                                                     int64_t ldp, int c0, int c1) {
  const int l = lane_id();
  const int64_t ti = (int64_t)blockIdx.x * P_WPB + (threadIdx.x >> 6);
  if (ti >= ntask) return;
  const pprprop::PTask tk = tasks[ti];
  const int c = c0 + ((int)blockIdx.y * WAVE + l) * V;
  const bool colok = c < c1;
  const int n = tk.n < 0 ? 0 : tk.n > pprprop::PROP_CHUNK ? pprprop::PROP_CHUNK : tk.n;
  double acc[V];
#pragma unroll
  for (int k = 0; k < V; k++) acc[k] = 0.0;
  for (int b = 0; b < n; b += WAVE) {
    int pos = -1;
    double wt = 0.0;
    const int64_t o = tk.off + b + l;
    if (b + l < n && o >= 0 && o < (int64_t)M) {
      const int64_t v = vals[o];
      const int64_t i = v >> P_JBITS;
      const int jj = (int)(v & ((1 << P_JBITS) - 1));
      if (i >= 0 && i < a.S) {
        const int u = p_src(s, a, i);
        const int slot = res_slot(a.part, a.sA, a.sB, u);
        if (jj < res_len(s, slot, u)) {
          const double sc = s.sc[s.row(slot, u) + jj];
          wt = a.norm ? pprprop::prop_weight(sc, wpos[i]) : sc;
          pos = (int)i;
        }
      }
    }
    p_gather<DT, V>(acc, pos, wt, 0, min(WAVE, n - b), Gm, ldg, c, colok);
  }
  if (!colok) return;
  if (tk.part < 0) {
    if (tk.key >= 0 && (int64_t)tk.key < s.n) p_store<DT, V>(Y, (int64_t)tk.key * ldy + c, acc);
  } else if (tk.part < nparts) {
#pragma unroll
    for (int k = 0; k < V; k++) parts[tk.part * ldp + (c - c0) + k] = acc[k];
  }
}

template <int DT>
__global__ void __launch_bounds__(P_THREADS) k_p_tfold(DevSlab s, const pprprop::PFold* folds, const double* parts,
                                                      int64_t nparts, int64_t ldp, void* Y, int64_t ldy, int c0,
                                                      int c1) {
  const pprprop::PFold f = folds[blockIdx.x];
  if (f.key < 0 || (int64_t)f.key >= s.n || f.part < 0 || f.m < 1 || f.part + f.m > nparts) return;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += P_THREADS) {
    double total = parts[f.part * ldp + (c - c0)];
    for (int m = 1; m < f.m; m++) total = total + parts[(f.part + m) * ldp + (c - c0)];
    p_store1<DT>(Y, (int64_t)f.key * ldy + c, total);
  }
}

// keys k0 + [0, nk) without postings: zero rows (one wave per key)
template <int DT>
__global__ void __launch_bounds__(P_THREADS) k_p_zero(const int32_t* kstart, int64_t nk, int64_t k0, void* Y, int64_t ldy,
                                                     int F) {
  const int64_t k = (int64_t)blockIdx.x * P_WPB + (threadIdx.x >> 6);
  if (k >= nk || kstart[k + 1] > kstart[k]) return;
  for (int c = lane_id(); c < F; c += WAVE) {
    if constexpr (DT == 0) reinterpret_cast<uint32_t*>(Y)[(k0 + k) * ldy + c] = 0u;
    else reinterpret_cast<uint16_t*>(Y)[(k0 + k) * ldy + c] = (uint16_t)0;
  }
}

}  // namespace pprk
