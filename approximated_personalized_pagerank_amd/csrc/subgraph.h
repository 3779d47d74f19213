// subgraph.h -- device code of the PPR-induced subgraph batches (ppr_grank_plan_subgraphs;
// subgraph.hip; host planning and the shared rules: subgraph_plan.h).
//
// A source's current row is ordered by (score descending, key ascending), the source's own key moved
// to the front on request, and cut at `size` entries: its members, with the ranks 0 .. c - 1. The
// induced edges are found by the sweep's walk over the members' adjacency lists, one read-only probe
// of a key -> rank table per edge. The walk is numbered: windows of 64 members, a window's edges in
// groups of 64 (subgraph_plan.h sg_groups). The count pass stores every group's hit count (a ballot)
// and adds to per-member integer counters; two scans turn them into rowptr and into every group's
// first output slot; the emit pass repeats the walk and writes each hit at its group's slot plus its
// lane's rank among the group's hits. No output position depends on the order of any atomic.
//
//   k_g_plan    one wave per row: decode, row_sort on the score bits, the root first, the cut; writes
//               the members and their score bits, the walk size W, the group count, the tier verdict
//   k_g_nodes   nodes / scores at their final offsets, in the caller's index type
//   k_g_wave    one wave per source, four per block, a 256-slot key -> rank table each
//   k_g_wg      one workgroup per source (one launch per table size): wave wv takes every 4th group
//   k_g_slice   one workgroup per (source, group range): the same walk, the same numbering
//   k_g_rowptr  rowptr in the caller's index type and the batch's edge_ptr words
#pragma once
#include "resident.h"
#include "subgraph_plan.h"

namespace pprk {

constexpr int G_WPB = 4;            // waves per k_g_wave block (and per k_g_plan block of narrow rows)
constexpr int G_WG_THREADS = 256;   // k_g_wg / k_g_slice
constexpr int G_FLAT_THREADS = 256; // k_g_nodes / k_g_rowptr

struct GArgs {
  // the rows: src, or src_base + q when null
  const int32_t* src;
  int64_t src_base;
  const uint8_t* part;
  int sA, sB;
  // the graph
  const int64_t* rp;
  const int32_t* colx;    // bit 31: the partition bit
  int64_t n;
  // the call
  int width;              // members kept at most = row stride of order / scb
  int root_first;
  int idx64;
  int64_t max_deg;
  // per source of the chunk
  int32_t* order;         // [nq][width] the members in rank order
  uint64_t* scb;          // [nq][width] their score bits
  int32_t* cnt;           // members
  int64_t* W;             // walked edges
  int64_t* ngr;           // groups of the walk
  int32_t* code;
  int32_t* capm;          // members max_deg silenced
  int32_t* rlen;          // decodable row entries
  const int64_t* noff;    // [nq + 1] batch id of the source's member 0 (global)
  const int64_t* goff;    // first group of the source within its walk batch
  int64_t* eptr;          // the source's first edge (global)
  // the walk batch
  int64_t nb0;            // batch id of the batch's first member
  int64_t ebase;          // edges before the batch
  unsigned long long* mc; // [Nb + 1] edges emitted per member
  const int64_t* roff;    // [Nb + 1] their exclusive scan
  int32_t* gcnt;          // [Gb + 1] hits per group
  const int32_t* gbase;   // [Gb + 1] their exclusive scan
  // the outputs (device memory of the caller; every store is checked against the capacities)
  int64_t node_cap, edge_cap;
  void* nodes;
  double* scores;
  void* rowptr;
  void* col;
  void* row;
  int64_t* eid;
};

struct GTable {           // key -> rank: keys in XTable's layout, a rank beside every key, the counters
  uint32_t* keys;
  uint16_t* rank;
  uint32_t* cnt;
  uint32_t mask;
};
__host__ __device__ constexpr int g_bins(int T) { return T < pprsubg::SG_MAX_WIDTH ? T : pprsubg::SG_MAX_WIDTH; }
__host__ __device__ constexpr size_t g_lds(int T) { return (size_t)T * 6 + (size_t)g_bins(T) * 4; }
__host__ __device__ constexpr size_t g_plan_lds(int Lp) { return (size_t)Lp * 12; }
__device__ __forceinline__ GTable g_carve(unsigned char* p, int T) {
  GTable t;
  t.keys = reinterpret_cast<uint32_t*>(p);
  t.rank = reinterpret_cast<uint16_t*>(p + (size_t)T * 4);
  t.cnt = reinterpret_cast<uint32_t*>(p + (size_t)T * 6);
  t.mask = (uint32_t)T - 1u;
  return t;
}

// a value of the caller's index type
__device__ __forceinline__ void g_put(void* base, int idx64, int64_t i, int64_t v) {
  if (idx64) reinterpret_cast<int64_t*>(base)[i] = v;
  else reinterpret_cast<int32_t*>(base)[i] = (int32_t)v;
}

// wave sum of 64-bit values; every lane active
__device__ __forceinline__ long long g_sum64(long long x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// ---------------------------------------------------------------------------------------------
template <bool HK>
__global__ void __launch_bounds__(G_WPB * WAVE) k_g_plan(DevSlab s, GArgs a, int64_t nq, int Lp, int64_t wave_max,
                                                          int64_t wg_max) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int wv = threadIdx.x >> 6, l = lane_id();
  const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (q >= nq) return;
  unsigned char* base = smem + (size_t)wv * g_plan_lds(Lp);
  uint64_t* rv = reinterpret_cast<uint64_t*>(base);
  int* rk = reinterpret_cast<int*>(base + (size_t)Lp * 8);
  const int64_t u = a.src ? (int64_t)a.src[q] : a.src_base + q;
  const int slot = res_slot(a.part, a.sA, a.sB, u);
  int len = res_len(s, slot, u);
  const int64_t r0 = s.row(slot, u);
  if (len > Lp) len = Lp;  // (the host sizes Lp to the row width)
  // ---- decode, compact (undecodable ids are skipped)
  int cnt = 0;
  for (int i0 = 0; i0 < len; i0 += WAVE) {
    const int i = i0 + l;
    int key = -1;
    uint64_t sb = 0;
    if (i < len) {
      key = res_key<HK>(s, s.ids[r0 + i]);
      if (key >= 0) sb = dbits(s.sc[r0 + i]);
    }
    const uint64_t mk = __ballot(key >= 0);
    if (key >= 0) {
      const int pos = cnt + __popcll(mk & lanemask_lt());
      rv[pos] = sb;
      rk[pos] = key;
    }
    cnt += __popcll(mk);
  }
  wave_fence();
  row_sort(rv, rk, cnt, Lp);
  // ---- the root's place in that order (-1: not asked for, or not in the row)
  int root = -1;
  if (a.root_first)
    for (int i0 = 0; i0 < cnt && root < 0; i0 += WAVE) {
      const int i = i0 + l;
      const uint64_t mk = __ballot(i < cnt && rk[i] == (int)u);
      if (mk) root = i0 + __ffsll((unsigned long long)mk) - 1;
    }
  // ---- the cut, the members, their walk
  const int keep = cnt < a.width ? cnt : a.width;
  const int64_t o = q * (int64_t)a.width;
  long long W = 0, ngr = 0;
  int capm = 0;
  for (int j0 = 0; j0 < keep; j0 += WAVE) {
    const int j = j0 + l;
    long long eff = 0;
    bool capped = false;
    if (j < keep) {
      const int si = root < 0 ? j : j == 0 ? root : j <= root ? j - 1 : j;  // (the root first, the others in order)
      const int key = rk[si];
      a.order[o + j] = key;
      a.scb[o + j] = rv[si];
      long long d = a.rp[key + 1] - a.rp[key];
      if (d < 0) d = 0;
      capped = a.max_deg > 0 && d > a.max_deg;
      eff = pprsubg::sg_eff_deg(d, a.max_deg);
    }
    const long long tot = g_sum64(eff);
    W += tot;
    ngr += pprsubg::sg_window_groups(tot);
    capm += __popcll(__ballot(capped));
  }
  if (l == 0) {
    a.cnt[q] = keep;
    a.W[q] = W;
    a.ngr[q] = ngr;
    a.capm[q] = capm;
    a.rlen[q] = cnt;
    a.code[q] = pprsubg::sg_tier(W, keep, wave_max, wg_max);
  }
}

// nodes / scores of a chunk at their final offsets: one thread per (source, rank)
__global__ void __launch_bounds__(G_FLAT_THREADS) k_g_nodes(GArgs a, int64_t nq) {
  const int64_t t = (int64_t)blockIdx.x * G_FLAT_THREADS + threadIdx.x;
  const int64_t q = t / a.width;
  const int j = (int)(t - q * a.width);
  if (q >= nq || j >= a.cnt[q]) return;
  const int64_t pos = a.noff[q] + j;
  if (pos >= a.node_cap) return;
  g_put(a.nodes, a.idx64, pos, a.order[t]);
  if (a.scores) a.scores[pos] = bitsd(a.scb[t]);
}

// ---- the key -> rank table of one source, cleared and filled by nthr threads (no barrier inside)
__device__ __forceinline__ void g_clear(const GTable& t, int T, int tid, int nthr) {
  for (int i = tid; i < T; i += nthr) t.keys[i] = 0u;
  for (int i = tid; i < g_bins(T); i += nthr) t.cnt[i] = 0u;
}
__device__ __forceinline__ bool g_fill(const GTable& t, const int32_t* ord, int cnt, int tid, int nthr) {
  bool bad = false;
  XTable xt;
  xt.keys = t.keys;
  xt.lo = nullptr;
  xt.hi = nullptr;
  xt.mask = t.mask;
  for (int i = tid; i < cnt; i += nthr) {
    bool ins;
    const int sl = xt_slot(xt, ord[i], ins);
    if (sl < 0) bad = true;
    else t.rank[sl] = (uint16_t)i;
  }
  return bad;
}

// The walk of source q, groups [g0, g1) of its numbering. Windows of 64 members: lane l holds member
// w0 + l's first edge and its edge count, a DPP scan numbers the window's edges, and every lane finds
// the member of its edge by the binary search over the scan (shuffles), so that consecutive lanes read
// consecutive words of an adjacency list. A window is never clipped: a range of the walk is a range of
// groups, so both passes and every tier give a group the same number and the same 64 edges. Wave wv
// of nw takes every nw-th group of a window's share. Per edge one probe; on a hit the count pass adds 1
// to the emitting member's counter (an integer LDS atomic: order-free) and lane 0 stores the group's hit
// count; the emit pass writes the edge at the group's first slot + the hits in lower lanes.
template <bool EMIT>
__device__ __forceinline__ void g_walk(const GArgs& a, const GTable& t, const int32_t* ord, int cnt, int64_t q, int64_t g0,
                                       int64_t g1, int wv, int nw) {
  const int l = lane_id();
  const int64_t G0 = a.goff[q], nbase = a.noff[q];
  int64_t gw = 0;  // groups of the windows before this one
  for (int w0 = 0; w0 < cnt && gw < g1; w0 += WAVE) {
    const int i = w0 + l;
    int n = 0;
    int64_t start = 0;
    if (i < cnt) {
      const int key = ord[i];
      start = a.rp[key];
      n = (int)pprsubg::sg_eff_deg(a.rp[key + 1] - start, a.max_deg);
    }
    const int incl = wave_incl_scan(n);
    const int total = __builtin_amdgcn_readlane(incl, WAVE - 1);  // (<= SG_EDGE_LIMIT: the host refuses more)
    const int ngw = (int)pprsubg::sg_window_groups(total);
    const int64_t lo = g0 > gw ? g0 - gw : 0, hi = g1 - gw < ngw ? g1 - gw : ngw;
    for (int64_t gi = lo + wv; gi < hi; gi += nw) {
      const int c = (int)gi * WAVE + l;
      int tl = 0;  // lanes whose scan is <= c: the first lane past them owns edge c
#pragma unroll
      for (int st = 32; st; st >>= 1) {
        const int v = __shfl(incl, tl + st - 1);
        tl += v <= c ? st : 0;
      }
      const int ex = __shfl(incl - n, tl);
      const long long st0 = __shfl((long long)start, tl);
      bool hit = false;
      int rb = 0;
      int64_t p = 0;
      if (c < total) {
        p = (int64_t)st0 + (c - ex);
        const int b = a.colx[p] & 0x7fffffff;
        const int m = res_find(t.keys, t.mask, b);
        if (m >= 0) {
          hit = true;
          rb = (int)t.rank[m];
        }
      }
      const uint64_t hits = __ballot(hit);
      const int64_t g = G0 + gw + gi;
      if (!EMIT) {
        if (l == 0) a.gcnt[g] = __popcll(hits);
        if (hit) atomicAdd(&t.cnt[w0 + tl], 1u);
      } else if (hit) {
        const int64_t pos = a.ebase + a.gbase[g] + __popcll(hits & lanemask_lt());
        if (pos < a.edge_cap) {
          g_put(a.col, a.idx64, pos, nbase + rb);
          if (a.row) g_put(a.row, a.idx64, pos, nbase + w0 + tl);
          if (a.eid) a.eid[pos] = p;
        }
      }
    }
    gw += ngw;
  }
}

// ---------------------------------------------------------------------------------------------
template <bool EMIT>
__global__ void __launch_bounds__(G_WPB * WAVE) k_g_wave(GArgs a, const int32_t* list, int64_t count) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int T = pprsubg::SG_WAVE_T;
  const int wv = threadIdx.x >> 6, l = lane_id();
  const int64_t w = (int64_t)blockIdx.x * G_WPB + wv;
  if (w >= count) return;
  const GTable t = g_carve(smem + (size_t)wv * g_lds(T), T);
  const int64_t q = list[w];
  int cnt = a.cnt[q];
  if (cnt > 3 * T / 4) { cnt = 0; if (l == 0) probe_fail(); }  // (cannot happen: sg_tier)
  const int32_t* ord = a.order + q * (int64_t)a.width;
  g_clear(t, T, l, WAVE);
  wave_fence();
  const bool bad = g_fill(t, ord, cnt, l, WAVE);
  wave_fence();
  if (__ballot(bad) && l == 0) probe_fail();
  g_walk<EMIT>(a, t, ord, cnt, q, 0, INT64_MAX, 0, 1);
  if (EMIT) return;
  wave_fence();
  unsigned long long* mc = a.mc + (a.noff[q] - a.nb0);
  for (int i = l; i < cnt; i += WAVE) mc[i] = t.cnt[i];
}

// the workgroup's table of one source; returns its members (0 and the error word when they cannot fit)
__device__ __forceinline__ int g_wg_table(const GArgs& a, const GTable& t, int T, int64_t q, const int32_t* ord) {
  int cnt = a.cnt[q];
  if (4 * cnt > 3 * T || cnt > g_bins(T)) { cnt = 0; if (threadIdx.x == 0) probe_fail(); }  // (cannot happen)
  g_clear(t, T, threadIdx.x, blockDim.x);
  __syncthreads();
  const bool bad = g_fill(t, ord, cnt, threadIdx.x, blockDim.x);
  if (__ballot(bad) && lane_id() == 0) probe_fail();
  __syncthreads();
  return cnt;
}

template <bool EMIT>
__global__ void __launch_bounds__(G_WG_THREADS) k_g_wg(GArgs a, const int32_t* list, int T) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int64_t q = list[blockIdx.x];
  const GTable t = g_carve(smem, T);
  const int32_t* ord = a.order + q * (int64_t)a.width;
  const int cnt = g_wg_table(a, t, T, q, ord);
  g_walk<EMIT>(a, t, ord, cnt, q, 0, INT64_MAX, threadIdx.x >> 6, blockDim.x >> 6);
  if (EMIT) return;
  __syncthreads();
  unsigned long long* mc = a.mc + (a.noff[q] - a.nb0);
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) mc[i] = t.cnt[i];
}

template <bool EMIT>
__global__ void __launch_bounds__(G_WG_THREADS) k_g_slice(GArgs a, const pprsubg::GTask* tasks) {
  extern __shared__ __align__(16) unsigned char smem[];
  const pprsubg::GTask tk = tasks[blockIdx.x];
  const int64_t q = tk.q;
  const int T = pprsubg::sg_table_slots(a.cnt[q]);
  const GTable t = g_carve(smem, T);
  const int32_t* ord = a.order + q * (int64_t)a.width;
  const int cnt = g_wg_table(a, t, T, q, ord);
  g_walk<EMIT>(a, t, ord, cnt, q, tk.g0, tk.g1, threadIdx.x >> 6, blockDim.x >> 6);
  if (EMIT) return;
  __syncthreads();
  unsigned long long* mc = a.mc + (a.noff[q] - a.nb0);  // (zeroed by the host; integer adds: order-free)
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const uint32_t h = t.cnt[i];
    if (h) atomicAdd(&mc[i], (unsigned long long)h);
  }
}

// rowptr of the batch's Nb members and the first edge of its nb sources (chunk indices b0 ..)
__global__ void __launch_bounds__(G_FLAT_THREADS) k_g_rowptr(GArgs a, int64_t b0, int64_t nb, int64_t Nb) {
  const int64_t t = (int64_t)blockIdx.x * G_FLAT_THREADS + threadIdx.x;
  if (t < Nb && a.rowptr) {
    const int64_t pos = a.nb0 + t;
    if (pos < a.node_cap) g_put(a.rowptr, a.idx64, pos, a.ebase + a.roff[t]);
  }
  if (t < nb) a.eptr[b0 + t] = a.ebase + a.roff[a.noff[b0 + t] - a.nb0];
}

}  // namespace pprk
