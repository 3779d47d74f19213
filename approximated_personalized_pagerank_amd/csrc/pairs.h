// pairs.h -- device code of the node-pair scores (ppr_grank_plan_pairs, pairs.hip).
//
// For a pair (u, v): the entry of v in B[u] (fwd, its rank in the row), the entry of u in B[v] (bwd),
// and the overlap of the two rows: |keys(B[u]) & keys(B[v])| and the exact dot product over the common
// keys (include/ppr_hip.h states the contract). Rows are stored by ascending hash_b(key) with a
// 64-range index (ppr_common.h), so a lookup is a probe of the one segment row_range(key) names, and
// the overlap of two rows is a walk of one against an LDS copy of the other.
//
//   k_p_len       one wave per listed node: its decodable entries (out_slen; out_clen of the lookup class)
//   k_p_rank      lookup class with ranks: one wave per group builds the row of u in LDS (p_build),
//                 sorts a copy by (score desc, key asc) and leaves every stored position's rank in HBM
//   k_p_look      lookup class: one lane per pair; v in the segment of B[u] and u in the segment of
//                 B[v], bounded through the rows' range indices exactly as k_r_probe bounds its own
//   k_p_ovl<NW>   overlap class: one task (a group's candidates [j0, j1)) per block of NW waves. The
//                 block builds B[u] in LDS -- keys and score bits in stored order, the 65 segment
//                 bounds, every position's rank when ranks are asked for -- and its waves take the
//                 candidates in turn: a wave streams B[v] in coalesced trips of 64 ids, each lane
//                 decodes its id, finds it in u's LDS segment (bisection or a linear scan), loads the
//                 score only on a hit and keeps a hit count and the 96-bit sum as three limbs
//                 (pairs_plan.h) in registers; one wave reduction per candidate finishes them. The
//                 lane whose key is u holds bwd; fwd and rank are one LDS lookup of v. NW = 1 is the
//                 wave tier, NW = P_WG_WAVES the workgroup tier and the tasks of split groups.
//
// Every output position is the pair's own; no float atomics; the sums are exact integers, so no
// result depends on the tier, the split, the chunking or the search. Every index derived from a
// length or a range-index entry is clamped to the row.
#pragma once
#include "pairs_plan.h"
#include "resident.h"

namespace pprk {

constexpr int P_WG_WAVES = 8;
constexpr int P_WG_THREADS = P_WG_WAVES * WAVE;
constexpr int P_LOOK_THREADS = 256;
constexpr int P_LEN_WPB = 4;  // k_p_len: waves (nodes) per block

struct PArgs {
  const uint8_t* part;
  int sA, sB;               // current slot of a partition-0 / partition-1 node
  uint32_t outs;            // pprpairs::PR_* bits
  int binary;               // the LDS search: bisection (1) or a linear scan (0)
  int Lp;                   // power of two >= L (the sort buffers of p_build)
  const int32_t* src;       // [groups of the chunk]
  const int32_t* cand;      // [pairs of the chunk]
  const int32_t* pg;        // [pairs] group of the pair (chunk index; lookup class)
  uint16_t* rankbuf;        // [groups * L] rank of every stored position (lookup class with ranks)
  double *fwd, *bwd, *dot;  // [pairs] each, or null
  uint8_t* hit;
  int32_t *rank, *common, *clen;
  unsigned long long* stat; // [0] row entries built in LDS / ranked, [1] candidate ids read, [2] hits, [3] / [4] entries k_p_len counted (sources / candidates), [5] forward hits (lookup)
};

// LDS of one p_build row: score bits [L] | sort values [Lp] | keys [L] | sort keys [Lp] | bounds [65 -> 68] | ranks [L] | counter
__host__ __device__ constexpr size_t p_lds(int L, int Lp, bool rank) {
  return (size_t)L * 8 + (rank ? (size_t)Lp * 8 : 0) + (size_t)L * 4 + (rank ? (size_t)Lp * 4 : 0) + 68 * 4 +
         (rank ? (((size_t)L * 2 + 15) & ~(size_t)15) : 0) + 16;
}
struct PRow {
  uint64_t* sc;    // score bits, stored order
  uint64_t* rv;    // sort buffer (ranks only)
  int* keys;       // decoded keys, stored order, -1 = undecodable
  int* rk;         // sort buffer
  int* sb;         // segment r = [sb[r], sb[r + 1])
  uint16_t* rank;  // rank of every stored position among the decodable entries
  int* cnt;        // [0] decodable entries
  int len;         // stored entries (clamped)
  bool binary;     // the segments may be bisected (every entry decodable)
};
__device__ __forceinline__ PRow p_carve(unsigned char* p, int L, int Lp, bool rank) {
  PRow r;
  r.sc = reinterpret_cast<uint64_t*>(p); p += (size_t)L * 8;
  r.rv = reinterpret_cast<uint64_t*>(p); p += rank ? (size_t)Lp * 8 : 0;
  r.keys = reinterpret_cast<int*>(p); p += (size_t)L * 4;
  r.rk = reinterpret_cast<int*>(p); p += rank ? (size_t)Lp * 4 : 0;
  r.sb = reinterpret_cast<int*>(p); p += 68 * 4;
  r.rank = reinterpret_cast<uint16_t*>(p); p += rank ? (((size_t)L * 2 + 15) & ~(size_t)15) : 0;
  r.cnt = reinterpret_cast<int*>(p);
  r.len = 0;
  r.binary = false;
  return r;
}

// position of `key` (in [0, n)) in the LDS row, or -1: its segment, bisected by hash_b or scanned
__device__ __forceinline__ int p_find(const PRow& r, int key) {
  const int rg = (int)row_range(key);
  const int b = r.sb[rg], e = r.sb[rg + 1];
  if (r.binary) {
    const uint32_t hk = hash_b((uint32_t)key);
    int lo = b, hi = e;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (hash_b((uint32_t)r.keys[mid]) < hk) lo = mid + 1; else hi = mid;
    }
    return lo < e && r.keys[lo] == key ? lo : -1;
  }
  for (int c = b; c < e; c++)
    if (r.keys[c] == key) return c;
  return -1;
}

// The block (nthr threads, a multiple of 64) builds the row of u. Ends with a barrier.
template <bool HK>
__device__ __forceinline__ void p_build(const DevSlab& s, const PArgs& a, PRow& r, int u, bool want_rank, int tid, int nthr) {
  const int slot = res_slot(a.part, a.sA, a.sB, u);
  const int len = res_len(s, slot, u);
  const int64_t row = s.row(slot, u), xr = s.xrow(slot, u);
  r.len = len;
  if (tid == 0) r.cnt[0] = 0;
  __syncthreads();
  int mine = 0;
  for (int c = tid; c < len; c += nthr) {
    const int key = res_key<HK>(s, s.ids[row + c]);
    r.keys[c] = key;
    r.sc[c] = dbits(s.sc[row + c]);
    mine += key >= 0 ? 1 : 0;
  }
  for (int q = tid; q <= NRANGE; q += nthr) {
    const int x = q == 0 ? 0 : q == NRANGE ? len : min((int)s.rix[xr + q - 1], len);
    r.sb[q] = x;
  }
  if (mine) atomicAdd(&r.cnt[0], mine);
  __syncthreads();
  const int dlen = r.cnt[0];
  // bisection needs every key of a segment in hash order: an undecodable entry (never on a sound slab) has none
  r.binary = a.binary && dlen == len;
  if (want_rank) {
    if (tid < WAVE) {  // wave 0: the decodable entries by (score desc, key asc), then every key back to its position
      int base = 0;
      for (int c0 = 0; c0 < len; c0 += WAVE) {
        const int c = c0 + tid;
        const int key = c < len ? r.keys[c] : -1;
        const uint64_t m = __ballot(key >= 0);
        if (key >= 0) {
          const int pos = base + __popcll(m & lanemask_lt());
          r.rv[pos] = r.sc[c];
          r.rk[pos] = key;
        }
        base += __popcll(m);
      }
      wave_fence();
      row_sort(r.rv, r.rk, dlen, a.Lp);
      for (int i = tid; i < dlen; i += WAVE) {
        const int c = p_find(r, r.rk[i]);
        if (c >= 0) r.rank[c] = (uint16_t)i;
      }
    }
    __syncthreads();
  }
}

// decodable entries of the listed nodes, one wave each
template <bool HK>
__global__ void __launch_bounds__(P_LEN_WPB * WAVE) k_p_len(DevSlab s, PArgs a, const int32_t* nodes, int64_t count, int32_t* out, int stat_slot) {
  const int64_t i = (int64_t)blockIdx.x * P_LEN_WPB + (threadIdx.x >> 6);
  if (i >= count) return;
  const int u = nodes[i];
  const int slot = res_slot(a.part, a.sA, a.sB, u);
  const int len = res_len(s, slot, u);
  const int64_t row = s.row(slot, u);
  int c = 0;
  for (int j = lane_id(); j < len; j += WAVE) c += res_key<HK>(s, s.ids[row + j]) >= 0 ? 1 : 0;
  c = wave_sum(c);
  if (lane_id() == 0) {
    out[i] = c;
    if (len) atomicAdd(&a.stat[stat_slot], (unsigned long long)len);
  }
}

// lookup class with ranks: the rank of every stored position of every group's row
template <bool HK>
__global__ void __launch_bounds__(WAVE) k_p_rank(DevSlab s, PArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  PRow r = p_carve(smem, s.L, a.Lp, true);
  const int g = blockIdx.x;
  p_build<HK>(s, a, r, a.src[g], true, threadIdx.x, WAVE);
  uint16_t* out = a.rankbuf + (int64_t)g * s.L;
  for (int c = threadIdx.x; c < r.len; c += WAVE) out[c] = r.keys[c] >= 0 ? r.rank[c] : (uint16_t)0;
  if (threadIdx.x == 0 && r.len) atomicAdd(&a.stat[0], (unsigned long long)r.len);
}

// position of `key` in the stored row of node x (global memory), or -1; `segs` counts the segment's ids
template <bool HK>
__device__ __forceinline__ int p_probe(const DevSlab& s, const PArgs& a, int x, int key, int64_t& row, unsigned long long& segs) {
  const int slot = res_slot(a.part, a.sA, a.sB, x);
  const int len = res_len(s, slot, x);
  const int64_t xr = s.xrow(slot, x);
  row = s.row(slot, x);
  const int rg = (int)row_range(key);
  const int b = rg > 0 ? min((int)s.rix[xr + rg - 1], len) : 0;
  const int e = rg < NRANGE - 1 ? min((int)s.rix[xr + rg], len) : len;
  segs += (unsigned long long)(e > b ? e - b : 0);
  for (int c = b; c < e; c++)
    if (res_key<HK>(s, s.ids[row + c]) == key) return c;  // (a row holds a key once)
  return -1;
}

template <bool HK>
__global__ void __launch_bounds__(P_LOOK_THREADS) k_p_look(DevSlab s, PArgs a, int64_t npairs) {
  const int64_t j = (int64_t)blockIdx.x * P_LOOK_THREADS + threadIdx.x;
  unsigned long long segs = 0ull, hits = 0ull, fh = 0ull;
  if (j < npairs) {
    const int g = a.pg[j];
    const int u = a.src[g], v = a.cand[j];
    int64_t ru, rv;
    const int cf = p_probe<HK>(s, a, u, v, ru, segs);
    const int cb = p_probe<HK>(s, a, v, u, rv, segs);
    hits = (cf >= 0 ? 1ull : 0ull) + (cb >= 0 ? 1ull : 0ull);
    fh = cf >= 0 ? 1ull : 0ull;
    if (a.fwd) a.fwd[j] = cf >= 0 ? s.sc[ru + cf] : 0.0;
    if (a.bwd) a.bwd[j] = cb >= 0 ? s.sc[rv + cb] : 0.0;
    if (a.hit) a.hit[j] = (uint8_t)((cf >= 0 ? 1 : 0) | (cb >= 0 ? 2 : 0));
    if (a.rank) a.rank[j] = cf >= 0 ? (int)a.rankbuf[(int64_t)g * s.L + cf] : -1;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    segs += __shfl_xor(segs, o);
    hits += __shfl_xor(hits, o);
    fh += __shfl_xor(fh, o);
  }
  if (lane_id() == 0) {
    if (segs) atomicAdd(&a.stat[1], segs);
    if (hits) atomicAdd(&a.stat[2], hits);
    if (fh) atomicAdd(&a.stat[5], fh);
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

template <bool HK, int NW>
__global__ void __launch_bounds__(NW * WAVE) k_p_ovl(DevSlab s, PArgs a, const pprpairs::PTask* tasks) {
  extern __shared__ __align__(16) unsigned char smem[];
  const bool want_rank = (a.outs & pprpairs::PR_RANK) != 0;
  const bool want_dot = (a.outs & pprpairs::PR_DOT) != 0;
  PRow r = p_carve(smem, s.L, a.Lp, want_rank);
  const pprpairs::PTask tk = tasks[blockIdx.x];
  const int u = a.src[tk.g];
  p_build<HK>(s, a, r, u, want_rank, threadIdx.x, NW * WAVE);
  const int wv = threadIdx.x >> 6, l = lane_id();
  unsigned long long ids_read = 0ull, hits = 0ull;
  for (int j = tk.j0 + wv; j < tk.j1; j += NW) {
    const int v = a.cand[j];
    const int slot = res_slot(a.part, a.sA, a.sB, v);
    const int len = res_len(s, slot, v);
    const int64_t row = s.row(slot, v);
    int common = 0, dl = 0;
    bool has_u = false;
    double bw = 0.0;
    pprpairs::Limbs acc{0ull, 0ull, 0ull};
    for (int c0 = 0; c0 < len; c0 += WAVE) {
      const int c = c0 + l;
      if (c >= len) continue;
      const int key = res_key<HK>(s, s.ids[row + c]);
      if (key < 0) continue;
      dl++;
      const int pos = p_find(r, key);
      const bool self = key == u;
      if (pos < 0 && !self) continue;
      double sv = 0.0;
      if (self || want_dot) sv = s.sc[row + c];
      if (self) { has_u = true; bw = sv; }
      if (pos >= 0) {
        common++;
        if (want_dot) {
          unsigned long long xl;
          uint32_t xh;
          xs_conv(bitsd(r.sc[pos]) * sv, xl, xh);  // a lone multiply: nothing to contract with
          acc = pprpairs::pr_add(acc, pprpairs::pr_split(xl, xh));
        }
      }
    }
    // one wave reduction per candidate (every lane is here again)
    const int ncommon = wave_sum(common);
    const int ndl = wave_sum(dl);
    const uint64_t um = __ballot(has_u);
    if (a.dot) {
      pprpairs::Limbs t;
      t.w0 = wave_sum_u64(acc.w0);
      t.w1 = wave_sum_u64(acc.w1);
      t.w2 = wave_sum_u64(acc.w2);
      unsigned long long lo;
      uint32_t hi;
      pprpairs::pr_join(t, lo, hi);
      if (l == 0) a.dot[j] = xs_to_double(hi, lo);
    }
    if (a.bwd) {
      const double b = um ? readlane_d(bw, __ffsll((long long)um) - 1) : 0.0;
      if (l == 0) a.bwd[j] = b;
    }
    if (l == 0) {
      const int pf = p_find(r, v);
      if (a.fwd) a.fwd[j] = pf >= 0 ? bitsd(r.sc[pf]) : 0.0;
      if (a.hit) a.hit[j] = (uint8_t)((pf >= 0 ? 1 : 0) | (um ? 2 : 0));
      if (a.rank) a.rank[j] = pf >= 0 ? (int)r.rank[pf] : -1;
      if (a.common) a.common[j] = ncommon;
      if (a.clen) a.clen[j] = ndl;
      ids_read += (unsigned long long)len;
      hits += (unsigned long long)ncommon;
    }
  }
  if (l == 0) {
    if (ids_read) atomicAdd(&a.stat[1], ids_read);
    if (hits) atomicAdd(&a.stat[2], hits);
    if (threadIdx.x == 0 && r.len) atomicAdd(&a.stat[0], (unsigned long long)r.len);
  }
}

}  // namespace pprk
