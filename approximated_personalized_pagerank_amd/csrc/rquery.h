// rquery.h -- device code of the reverse queries (ppr_grank_plan_rquery, rquery.hip).
//
// The forward query (query.h) is the vector-matrix product f^T B over a few rows of the resident
// basket table B; this is the other direction, the matrix-vector product B f: for a weighted target
// set, which sources rank it highest. For query q with targets t_j and factors f_j = w_j / W
//     X_q[u] = sum_j [t_j in B[u]] floor(fl(B[u][t_j] * f_j) * 2^93)
// an exact integer sum (xs_table.h), score(u) = X_q[u] * 2^-93 rounded once; u is a hit of q when at
// least one target of q is a key of B[u] (a zero score is a legal hit); the Kq best hits by (score
// desc, source id asc) go to the caller, the same rule at the cut (TieIdAsc). The table is stored by
// rows, so a column lookup is a scan of the rows' ids -- 4 * sum len[u] bytes -- or, for a handful of
// postings, a probe of every row through its 64-range index. Postings = the (query, target, f)
// triples of a chunk of queries.
//
//   k_r_scan<EMIT>  the scan tier. Every workgroup holds the chunk's target table in LDS (decoded key
//                   -> index of the distinct target; tptr / pq / pf give its postings). A sub-wave
//                   of G lanes owns a row and loads its ids (16 B per lane when L % 4 == 0); most
//                   rows hit nothing and end there. The hits of a row are packed into a per-wave LDS
//                   buffer, and the whole wave sums the row per query: one posting is a direct emit,
//                   up to R_WCAP postings go through a 64-slot per-wave XTable keyed by the query
//                   index, more send the row to the overflow list. EMIT = false counts hits per query
//                   (no score is read), EMIT = true appends (u, score) to the query's list at offsets
//                   the host derived from the counts.
//   k_r_ovf<EMIT>   one workgroup per overflow row, an XTable of up to T slots
//   k_r_probe       the probe tier: one lane per row, every posting of the chunk in turn through the
//                   row's range index, 96-bit sums in registers, lists of n entries per query
//   k_r_seg         one wave per segment of a long list: its top-Kq goes to the next level (the
//                   top-Kq of disjoint sets lies in the union of theirs, as k_q_range / k_q_final)
//   k_r_final       one wave per query: top-Kq of what is left, sorted, the result row
//
// No table can fill, by construction (the host cuts the call into chunks of at most 3/4 T postings):
//   target table    distinct targets <= postings <= 3/4 T, and its image has >= 4/3 distinct slots;
//   per-wave table  a row goes there only with <= R_WCAP = 3/4 * 64 postings, and the distinct
//                   queries of a row are at most its postings;
//   overflow table  the distinct queries that can hit one row are <= min(postings, queries of the
//                   chunk) <= 3/4 of its slots.
// A probe that runs out anyway sets g_probe_err (PPR_ERR_PROBE). Every tier computes the same exact
// totals and one total order decides every cut: the result depends only on the slab and the query.
// The helpers shared with the forward queries and the propagation (slot, length, id decode, the
// read-only table probe, select-and-compact, the result row) are in resident.h.
#pragma once
#include "resident.h"

namespace pprk {

constexpr int R_MAX_K = 4096;
constexpr int R_MIN_T = 256, R_MAX_T = 8192;
constexpr int R_SCAN_THREADS = 512;   // k_r_scan: 8 waves share one LDS copy of the target table
constexpr int R_WT = 64;              // per-wave table slots (one per lane)
constexpr int R_WCAP = 3 * R_WT / 4;  // postings of a row summed in the wave
constexpr int R_HB = 256;             // per-wave hit buffer: 64 lanes x 4 ids of one trip
constexpr int R_OVF_THREADS = 256;
constexpr int R_PROBE_THREADS = 256;
constexpr int R_WPB = 4;              // waves per k_r_seg block
constexpr uint32_t R_DROPPED = 0xffffffffu;  // high word of an excluded (query, source): no total reaches it
// Hit counters. Global atomics execute at the memory side, and adds to one address -- or to the few
// lines of a dense counter array -- queue up in one channel (a key that sits in 1.9 M of the RMAT-22
// rows cost 21 ms per pass that way). So a query's list is cut into 1 << lgS sub-lists, a hit source u
// goes to sub-list hash32(u) mod 2^lgS (a function of the row: the same in the count and the emit
// pass), and every counter has 256 B to itself (R_CSTRIDE ints apart).
constexpr int R_CSTRIDE = 64;
constexpr int R_MAX_LGS = 6;

struct RArgs {
  const uint8_t* part;
  int sA, sB;             // current slot of a partition-0 / partition-1 node
  int Kq;
  uint32_t exclude;       // PPR_RQUERY_EXCLUDE_TARGETS
  int nq;                 // queries of the chunk
  // the chunk's queries in query order (probe tier)
  const int64_t* qptr;    // [nq + 1]
  const int32_t* targets;
  const double* fac;      // f_j = w_j / W
  // the chunk's target table and the target -> postings CSR (scan tier)
  const uint32_t* tkeys;  // [Tt] key + 1, 0 = empty; groups of four, as XTable
  const uint32_t* tvals;  // [Tt] index of the distinct target
  int Tt;
  const int32_t* tptr;    // [distinct + 1]
  const int32_t* pq;      // [postings] query (chunk index)
  const double* pf;       // [postings] factor
  // hit counts and lists; counter c = (query << lgS) | sub-list
  int lgS;
  int32_t* hits;          // [c * R_CSTRIDE] hit sources (count pass; the capacity of the sub-list)
  const int64_t* loff;    // [c] offset of the sub-list, -1 = not in this emit batch
  int32_t* lcnt;          // [c * R_CSTRIDE] entries appended
  int32_t* lk;
  double* lv;
  int32_t* ovf;           // [n] overflow rows
  int32_t* ovf_cnt;
  unsigned long long* stat;  // [0] sum of len over the rows (count pass), [1] segment ids read (probe)
};

struct RSeg {             // one k_r_seg / k_r_final wave
  int64_t in_off, out_off;  // entries [in_off, in_off + n) -> [out_off, out_off + min(n, Kq)) | unused
  int32_t n;
  int32_t q;              // chunk index of the query (k_r_final)
};

__host__ __device__ constexpr size_t r_wave_lds() { return xt_bytes(R_WT) + (size_t)R_HB * 4; }
__host__ __device__ constexpr size_t r_scan_lds(int Tt) {
  return (size_t)Tt * 8 + (R_SCAN_THREADS / 64) * r_wave_lds();
}
__host__ __device__ constexpr size_t r_final_lds(int Kp) { return (size_t)Kp * 12 + 1024; }

// index of the distinct target `key` (in [0, n)) or -1: the image is never more than 3/4 full
__device__ __forceinline__ int r_lookup(const uint32_t* tk, const uint32_t* tv, int Tt, int key) {
  const int m = res_find(tk, (uint32_t)Tt - 1u, key);
  return m >= 0 ? (int)tv[m] : -1;
}

// mark query q of the table dropped (its source is one of its targets)
__device__ __forceinline__ void r_drop(const XTable& t, int q) {
  const int m = res_find(t.keys, t.mask, q);
  if (m >= 0) t.hi[m] = R_DROPPED;
}

// one (query, source) hit: counted, or appended to the query's list (any order: the final order is total)
template <bool EMIT>
__device__ __forceinline__ void r_emit(const RArgs& a, int q, int u, double score) {
  const int64_t c = ((int64_t)q << a.lgS) | (int64_t)(hash32((uint32_t)u) & ((1u << a.lgS) - 1u));
  if (!EMIT) {
    atomicAdd(&a.hits[c * R_CSTRIDE], 1);
    return;
  }
  const int64_t o = a.loff[c];
  if (o < 0) return;  // another emit batch
  const int pos = atomicAdd(&a.lcnt[c * R_CSTRIDE], 1);
  if (pos >= a.hits[c * R_CSTRIDE]) {  // (cannot happen: the count pass walked the same rows)
    probe_fail();
    return;
  }
  a.lk[o + pos] = u;
  a.lv[o + pos] = score;
}

__device__ __forceinline__ void r_overflow(const DevSlab& s, const RArgs& a, int u) {
  if (lane_id() == 0) {
    const int pos = atomicAdd(a.ovf_cnt, 1);
    if ((int64_t)pos < s.n) a.ovf[pos] = u; else probe_fail();  // (a row overflows once per pass)
  }
}

// hit buffer word: row of the wave's window << 25 | position in the row << 13 | distinct target
__device__ __forceinline__ uint32_t r_pack(int r, int c, int d) { return ((uint32_t)r << 25) | ((uint32_t)c << 13) | (uint32_t)d; }

// One wave: row u (entries at `row`) with the hits hb[b .. e): sum per query, then count or emit.
template <bool EMIT>
__device__ __forceinline__ void r_row(const DevSlab& s, const RArgs& a, const uint32_t* tk, const uint32_t* tv,
                                      const XTable& wt, const uint32_t* hb, int u, int64_t row, int b, int e,
                                      bool over) {
  const int l = lane_id();
  if (over) { r_overflow(s, a, u); return; }
  int P = 0;
  for (int i = b + l; i < e; i += WAVE) {
    const int d = (int)(hb[i] & 0x1fffu);
    P += a.tptr[d + 1] - a.tptr[d];
  }
  P = wave_sum(P);
  if (P > R_WCAP) { r_overflow(s, a, u); return; }
  int xb = 0, xe = 0;  // the postings of u itself, when it is a target: the queries that drop it
  if (a.exclude) {
    const int du = r_lookup(tk, tv, a.Tt, u);
    if (du >= 0) { xb = a.tptr[du]; xe = a.tptr[du + 1]; }
  }
  if (P == 1) {  // (e - b == 1: every target has a posting)
    const uint32_t w = hb[b];
    const int p = a.tptr[w & 0x1fffu];
    const int q = a.pq[p];
    bool ex = false;
    for (int i = xb + l; i < xe; i += WAVE) ex |= a.pq[i] == q;
    if (__ballot(ex)) return;
    if (l == 0) r_emit<EMIT>(a, q, u, EMIT ? xs_single(s.sc[row + ((w >> 13) & 0xfffu)] * a.pf[p]) : 0.0);
    return;
  }
  wt.keys[l] = 0u; wt.lo[l] = 0ull; wt.hi[l] = 0u;
  wave_fence();
  bool bad = false;
  for (int i = b; i < e; i++) {
    const uint32_t w = hb[i];
    const int d = (int)(w & 0x1fffu);
    const int pb = a.tptr[d], pe = a.tptr[d + 1];
    const double sv = EMIT ? s.sc[row + ((w >> 13) & 0xfffu)] : 0.0;
    for (int p = pb + l; p < pe; p += WAVE) {
      unsigned long long lo = 0ull;
      uint32_t hi = 0u;
      if (EMIT) xs_conv(sv * a.pf[p], lo, hi);  // a lone multiply: nothing to contract with
      if (xt_add(wt, a.pq[p], lo, hi) < 0) bad = true;
    }
  }
  wave_fence();
  if (__ballot(bad) && l == 0) probe_fail();
  for (int i = xb + l; i < xe; i += WAVE) r_drop(wt, a.pq[i]);
  wave_fence();
  const uint32_t kt = wt.keys[l];
  const uint32_t hi = wt.hi[l];
  if (kt != 0u && hi != R_DROPPED) r_emit<EMIT>(a, (int)kt - 1, u, EMIT ? xs_to_double(hi, wt.lo[l]) : 0.0);
  wave_fence();
}

// V = ids per load (4: 16-B loads, L % 4 == 0 keeps every row 16-B aligned; 1 otherwise). G = lanes
// per row = 1 << lgG = min(64, the power of two >= ceil(L / V)): with G < 64 a row takes one trip and
// a wave walks 64 / G rows at once; with G = 64 a wave owns one row and takes ceil(len / (64 V)) trips.
template <bool EMIT, int V>
__global__ void __launch_bounds__(R_SCAN_THREADS) k_r_scan(DevSlab s, RArgs a, int lgG, int64_t nwin) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint32_t* tk = reinterpret_cast<uint32_t*>(smem);
  uint32_t* tv = tk + a.Tt;
  const int wv = threadIdx.x >> 6, nwv = R_SCAN_THREADS / WAVE;
  unsigned char* wbase = smem + (size_t)a.Tt * 8 + (size_t)wv * r_wave_lds();
  const XTable wt = xt_carve(wbase, R_WT);
  uint32_t* hb = reinterpret_cast<uint32_t*>(wbase + xt_bytes(R_WT));
  for (int i = threadIdx.x; i < a.Tt; i += R_SCAN_THREADS) { tk[i] = a.tkeys[i]; tv[i] = a.tvals[i]; }
  __syncthreads();
  const int l = lane_id(), G = 1 << lgG, R = WAVE >> lgG, r = l >> lgG, j = l & (G - 1);
  unsigned long long lensum = 0ull;
  for (int64_t w = (int64_t)blockIdx.x * nwv + wv; w < nwin; w += (int64_t)gridDim.x * nwv) {
    const int64_t u = w * R + r;
    int len = 0;
    int64_t row = 0;
    if (u < s.n) {
      const int slot = res_slot(a.part, a.sA, a.sB, u);
      len = res_len(s, slot, u);
      row = s.row(slot, u);
    }
    if (!EMIT && j == 0) lensum += (unsigned long long)len;
    int maxlen = len;
#pragma unroll
    for (int o = 32; o; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
    int nhb = 0, nh = 0, incl = 0;  // hits buffered | this lane's, their scan (the last trip's)
    for (int c0 = 0; c0 < maxlen; c0 += G * V) {
      const int c = c0 + j * V;
      int hv[V];
#pragma unroll
      for (int k = 0; k < V; k++) hv[k] = -1;
      if (c < len) {
        int32_t id[V];
        if (V == 4) {
          const int4 x = *reinterpret_cast<const int4*>(s.ids + row + c);
          id[0] = x.x; id[1 % V] = x.y; id[2 % V] = x.z; id[3 % V] = x.w;
        } else {
          id[0] = s.ids[row + c];
        }
#pragma unroll
        for (int k = 0; k < V; k++) {
          if (c + k < len) {
            const int key = res_key<true>(s, id[k]);
            if (key >= 0) hv[k] = r_lookup(tk, tv, a.Tt, key);
          }
        }
      }
      nh = 0;
#pragma unroll
      for (int k = 0; k < V; k++) nh += hv[k] >= 0 ? 1 : 0;
      incl = wave_incl_scan(nh);
      const int tot = __builtin_amdgcn_readlane(incl, WAVE - 1);
      if (tot) {
        int pos = nhb + incl - nh;
#pragma unroll
        for (int k = 0; k < V; k++)
          if (hv[k] >= 0) {
            if (pos < R_HB) hb[pos] = r_pack(r, c + k, hv[k]);
            pos++;
          }
        nhb += tot;
      }
    }
    if (nhb == 0) continue;
    wave_fence();
    if (lgG == 6) {
      r_row<EMIT>(s, a, tk, tv, wt, hb, (int)w, __shfl((long long)row, 0), 0, nhb < R_HB ? nhb : R_HB, nhb > R_HB);
    } else {  // one trip: at most 64 V <= R_HB hits, grouped by row (a row's lanes are adjacent)
      uint64_t m = __ballot(nh > 0);
      while (m) {
        const int rr = (__ffsll((long long)m) - 1) >> lgG;
        m &= ~(((1ull << G) - 1ull) << (rr << lgG));
        const int b = __shfl(incl - nh, rr << lgG), e = __shfl(incl, (rr << lgG) + G - 1);
        r_row<EMIT>(s, a, tk, tv, wt, hb, (int)(w * R + rr), __shfl((long long)row, rr << lgG), b, e, false);
      }
    }
  }
  if (!EMIT) {
#pragma unroll
    for (int o = 32; o; o >>= 1) lensum += __shfl_xor(lensum, o);
    if (l == 0 && lensum) atomicAdd(&a.stat[0], lensum);
  }
}

// One workgroup per overflow row: the whole row again, into a table of T slots keyed by the query.
// The target table is read from its image in HBM (a rare path; T slots of sums take the LDS).
template <bool EMIT>
__global__ void __launch_bounds__(R_OVF_THREADS) k_r_ovf(DevSlab s, RArgs a, int T) {
  extern __shared__ __align__(16) unsigned char smem[];
  const XTable t = xt_carve(smem, T);
  const int tid = threadIdx.x;
  const int u = a.ovf[blockIdx.x];
  for (int i = tid; i < T; i += R_OVF_THREADS) { t.keys[i] = 0u; t.lo[i] = 0ull; t.hi[i] = 0u; }
  __syncthreads();
  const int slot = res_slot(a.part, a.sA, a.sB, u);
  const int len = res_len(s, slot, u);
  const int64_t row = s.row(slot, u);
  bool bad = false;
  for (int c = tid; c < len; c += R_OVF_THREADS) {
    const int key = res_key<true>(s, s.ids[row + c]);
    const int d = key >= 0 ? r_lookup(a.tkeys, a.tvals, a.Tt, key) : -1;
    if (d < 0) continue;
    const double sv = EMIT ? s.sc[row + c] : 0.0;
    for (int p = a.tptr[d]; p < a.tptr[d + 1]; p++) {
      unsigned long long lo = 0ull;
      uint32_t hi = 0u;
      if (EMIT) xs_conv(sv * a.pf[p], lo, hi);
      if (xt_add(t, a.pq[p], lo, hi) < 0) bad = true;
    }
  }
  if (bad) probe_fail();
  __syncthreads();
  if (a.exclude) {
    const int du = r_lookup(a.tkeys, a.tvals, a.Tt, u);
    if (du >= 0)
      for (int i = a.tptr[du] + tid; i < a.tptr[du + 1]; i += R_OVF_THREADS) r_drop(t, a.pq[i]);
    __syncthreads();
  }
  for (int i = tid; i < T; i += R_OVF_THREADS) {
    const uint32_t kt = t.keys[i];
    const uint32_t hi = t.hi[i];
    if (kt != 0u && hi != R_DROPPED) r_emit<EMIT>(a, (int)kt - 1, u, EMIT ? xs_to_double(hi, t.lo[i]) : 0.0);
  }
}

// Probe tier: one lane per row. The postings loops are the same for every lane (scalar loads of the
// targets and factors); a target is searched in the segment of its key range, which the row's range
// index bounds. List of query q: n entries at loff[q] (a query cannot have more hits than rows); one
// counter per query (lgS = 0: the compiler folds a wave's adds to one address into one).
__global__ void __launch_bounds__(R_PROBE_THREADS) k_r_probe(DevSlab s, RArgs a) {
  const int64_t u = (int64_t)blockIdx.x * R_PROBE_THREADS + threadIdx.x;
  const bool live = u < s.n;
  int len = 0;
  int64_t row = 0, xr = 0;
  if (live) {
    const int slot = res_slot(a.part, a.sA, a.sB, u);
    len = res_len(s, slot, u);
    row = s.row(slot, u);
    xr = s.xrow(slot, u);
  }
  unsigned long long segs = 0ull;
  for (int q = 0; q < a.nq; q++) {
    const int64_t jb = a.qptr[q], je = a.qptr[q + 1];
    if (jb == je) continue;
    unsigned long long lo = 0ull;
    uint32_t hi = 0u;
    bool hit = false, self = false;
    for (int64_t j = jb; j < je; j++) {
      const int t = a.targets[j];
      self |= (int64_t)t == u;
      if (!live) continue;
      const int rg = (int)row_range(t);
      const int b = rg > 0 ? min((int)s.rix[xr + rg - 1], len) : 0;
      const int e = rg < NRANGE - 1 ? min((int)s.rix[xr + rg], len) : len;
      segs += (unsigned long long)(e > b ? e - b : 0);
      for (int c = b; c < e; c++) {
        if (res_key<true>(s, s.ids[row + c]) != t) continue;
        unsigned long long xl;
        uint32_t xh;
        xs_conv(s.sc[row + c] * a.fac[j], xl, xh);  // a lone multiply
        const unsigned long long old = lo;
        lo += xl;
        hi += xh + (lo < old ? 1u : 0u);
        hit = true;
        break;  // (a row holds a key once)
      }
    }
    if (hit && !(a.exclude && self)) {
      const int pos = atomicAdd(&a.lcnt[(int64_t)q * R_CSTRIDE], 1);
      if ((int64_t)pos < s.n) {
        a.lk[a.loff[q] + pos] = (int)u;
        a.lv[a.loff[q] + pos] = xs_to_double(hi, lo);
      } else {
        probe_fail();
      }
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) segs += __shfl_xor(segs, o);
  if (lane_id() == 0 && segs) atomicAdd(&a.stat[1], segs);
}

// One wave per segment: its min(n, Kq) best by (score desc, id asc) go to the next level's list.
__global__ void __launch_bounds__(R_WPB * WAVE) k_r_seg(const RSeg* tasks, int64_t ntask, int32_t* lk, double* lv, int Kq) {
  __shared__ uint32_t hist_all[R_WPB][256];
  const int wv = threadIdx.x >> 6;
  const int64_t ti = (int64_t)blockIdx.x * R_WPB + wv;
  if (ti >= ntask) return;
  uint32_t* hist = hist_all[wv];
  const RSeg tk = tasks[ti];
  const int n = tk.n;
  const int32_t* ik = lk + tk.in_off;
  const double* iv = lv + tk.in_off;
  int32_t* ok = lk + tk.out_off;
  double* ov = lv + tk.out_off;
  wave_select_compact(n, Kq, [&](int i) { return ik[i]; }, [&](int i) { return iv[i]; }, hist,
                      [&](int pos, int key, uint64_t vb) { ok[pos] = key; ov[pos] = bitsd(vb); });
}

// One wave per query: the top-Kq of its (reduced) list, sorted (score desc, id asc), unused slots
// id -1 / score 0 (write_result_row).
__global__ void __launch_bounds__(WAVE) k_r_final(const RSeg* tasks, const int32_t* lk, const double* lv, int Kq, int Kp,
                                                  int32_t* out_ids, double* out_sc, int32_t* out_len) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint64_t* rv = reinterpret_cast<uint64_t*>(smem);
  int* rk = reinterpret_cast<int*>(smem + (size_t)Kp * 8);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + (size_t)Kp * 12);
  const RSeg tk = tasks[blockIdx.x];
  const int n = tk.n;
  const int32_t* ik = lk + tk.in_off;
  const double* iv = lv + tk.in_off;
  const int cnt = wave_select_compact(n, Kq, [&](int i) { return ik[i]; }, [&](int i) { return iv[i]; }, hist,
                                      [&](int pos, int key, uint64_t vb) { rv[pos] = vb; rk[pos] = key; });
  wave_fence();
  write_result_row(out_ids, out_sc, out_len, tk.q, Kq, rv, rk, cnt, Kp);
}

}  // namespace pprk
