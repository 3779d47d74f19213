// query.h -- device code of the preference-set queries (ppr_grank_plan_query, query.hip).
//
// By the linearity of PPR (Jeh & Widom) the vector personalised to a weighted seed set is the
// weighted sum of the seeds' own vectors: PPR(sum_i f_i e_{u_i}) = sum_i f_i PPR(u_i). The plan
// holds every node's L-wide basket B[u] in HBM, so a query is one more basket merge:
//     total[k] = sum_i sum_{(k, s) in B[u_i]} floor(fl(s * f_i) * 2^93)
// an exact integer sum (xs_table.h: order-free, so any lane, wave or workgroup adds with LDS
// atomics), rounded once to a double, and the Kq best (score desc, dense id asc) go to the caller.
// One factor per seed, no self term, no slab write, no norm1: the GRank walk (hub_window_walk,
// finish_source) does not apply. A tie at the Kq-th place goes to the smaller id (TieIdAsc): the
// per-source tie hash de-biases an iterated top-L, and a query feeds nothing back.
//
//   k_q_plan    one wave per query: candidates C = sum len[u_i], the candidates of each of the 64
//               key ranges from the rows' range index (128 B per seed, no row touched), and from
//               them the tier: wave (C <= 3/4 T, T = 256 .. 2048), workgroup (C <= 3/4 T, T up to
//               8192), or the smallest power-of-two split R <= 64 whose every range group has at
//               most 3/4 T candidates. Distinct keys <= candidates, so no table can fill.
//   k_q_wave    one wave per query, four per block, LDS table of 256 << class slots
//   k_q_wg      one workgroup per query, a shared table (one launch per table size); the seeds are
//               spread over the waves
//   k_q_range   one workgroup per (query, range group): reads from each seed row only the
//               contiguous segment of its group (rows are in hash_b order) and appends its top-Kq
//               to the query's list -- the top-Kq of disjoint key sets lies in the union of theirs
//   k_q_final   one wave per split query: top-Kq of its list
// The result depends only on the slab and the query: every tier computes the same exact totals and
// the same total order decides every cut.
// The helpers shared with the reverse queries and the propagation (slot, length, id decode, the
// read-only table probe, select-and-compact, the result row) are in resident.h.
#pragma once
#include "resident.h"

namespace pprk {

constexpr int Q_WAVE_CLASSES = 4;      // wave-tier tables: 256 << class slots
constexpr int Q_WPB = 4;               // waves per k_q_wave / k_q_plan block
constexpr int Q_WG_THREADS = 256;      // k_q_wg / k_q_range
constexpr int Q_MAX_K = 4096;
constexpr int Q_MIN_T = 256, Q_MAX_T = 8192;
// planner verdict of one query: wave class 0..3 | Q_CODE_WG + log2 T | Q_CODE_RANGE + log2 R | too wide
constexpr int Q_CODE_WG = 0x100, Q_CODE_RANGE = 0x200, Q_CODE_WIDE = -1;
constexpr int Q_SAT = 1 << 24;         // per-range counts saturate here (far above any table)

struct QArgs {
  const int64_t* qptr;   // [nq + 1] offsets of the chunk's queries into seeds / fac (qptr[0] = 0)
  const int32_t* seeds;  // dense ids, checked on the host
  const double* fac;     // f_i = w_i / W
  const uint8_t* part;
  int sA, sB;            // current slot of a partition-0 / partition-1 node
  int Kq;
  uint32_t exclude;      // PPR_QUERY_EXCLUDE_SEEDS
  int32_t* out_ids;      // [nq][Kq]
  double* out_sc;
  int32_t* out_len;      // [nq]
};

struct QTask {           // one k_q_range workgroup
  int32_t q;             // query (chunk index)
  int32_t rq;            // its list
  int32_t g, R;          // range group g of R
};

struct QLists {          // appended top-Kq of the range groups, one list per split query
  const int64_t* off;    // [nrq + 1]
  int32_t* cnt;          // [nrq] entries appended (zeroed before the launch)
  int32_t* k;
  double* v;
};

__host__ __device__ constexpr size_t q_wave_lds(int T) { return (size_t)T * 16 + 1024; }
__host__ __device__ constexpr size_t q_final_lds(int Kp) { return (size_t)Kp * 12 + 1024; }

// Add the segments [range r0, range r1) of the rows of seeds [sb, se) into the table. Wave wv of nw
// takes every nw-th window of 64 seeds: lane l holds seed l's segment start, length and factor, a
// scan of the lengths numbers the window's candidates, and every lane finds the seed of its
// candidate by a binary search over the scan (shuffles) -- a row of one entry (a dangling node's)
// costs one lane, not a trip. Every row index stays inside [0, len[u]). Returns true when a probe
// ran out (a sizing error: the planner bounds the candidates by 3/4 of the slots).
__device__ __forceinline__ bool q_accumulate(const DevSlab& s, const QArgs& qa, int64_t sb, int64_t se, int r0,
                                             int r1, const XTable& t, int wv, int nw) {
  bool bad = false;
  const int l = lane_id();
  for (int64_t w0 = sb + (int64_t)wv * WAVE; w0 < se; w0 += (int64_t)nw * WAVE) {
    const int64_t i = w0 + l;
    int n = 0;
    int64_t start = 0;
    double f = 0.0;
    if (i < se) {
      const int u = qa.seeds[i];
      const int slot = res_slot(qa.part, qa.sA, qa.sB, u);
      const int len = res_len(s, slot, u);
      int b = 0, e = len;
      if (r0 > 0) b = min((int)s.rix[s.xrow(slot, u) + r0 - 1], len);
      if (r1 < NRANGE) e = min((int)s.rix[s.xrow(slot, u) + r1 - 1], len);
      if (e < b) e = b;
      n = e - b;
      start = s.row(slot, u) + b;
      f = qa.fac[i];
    }
    const int incl = wave_incl_scan(n);
    const int total = __builtin_amdgcn_readlane(incl, WAVE - 1);
    for (int c0 = 0; c0 < total; c0 += WAVE) {
      const int c = c0 + l;
      int tl = 0;  // lanes whose scan is <= c: the first lane past them owns candidate c
#pragma unroll
      for (int st = 32; st; st >>= 1) {
        const int v = __shfl(incl, tl + st - 1);
        tl += v <= c ? st : 0;
      }
      const int ex = __shfl(incl - n, tl);
      const long long st0 = __shfl((long long)start, tl);
      const double ft = __shfl(f, tl);
      if (c < total) {
        const int64_t a = (int64_t)st0 + (c - ex);
        const int32_t id = s.ids[a];
        const int key = res_key<true>(s, id);  // (hot-tagged ids exist after a chain-mode run)
        const double p = s.sc[a] * ft;  // a lone multiply: nothing to contract with
        unsigned long long lo;
        uint32_t hi;
        xs_conv(p, lo, hi);
        // (key < 0, written as res_key's own compare: one instruction for both)
        if ((uint32_t)key >= (uint32_t)s.n || xt_add(t, key, lo, hi) < 0) bad = true;
      }
    }
  }
  return bad;
}

// PPR_QUERY_EXCLUDE_SEEDS: every seed's slot (if the key is in the table) gets the high word
// 0xffffffff -- no total reaches it (X < 2^95) -- and q_select drops such slots.
constexpr uint32_t Q_DROPPED = 0xffffffffu;
__device__ __forceinline__ void q_exclude(const XTable& t, const QArgs& qa, int64_t sb, int64_t se, int tid, int nthr) {
  for (int64_t i = sb + tid; i < se; i += nthr) {
    const int m = res_find(t.keys, t.mask, qa.seeds[i]);
    if (m >= 0) t.hi[m] = Q_DROPPED;
  }
}

// One wave: settle the table's totals and keep the Kq best by (score desc, id asc), in place over
// the front of the table's arrays (rv = score bits over lo, rk = keys over keys). Returns the
// number kept = min(Kq, distinct keys left). The kept entries are in no particular order.
__device__ __forceinline__ int q_select(const XTable& t, int T, int Kq, uint32_t* hist) {
  double* vals = reinterpret_cast<double*>(t.lo);
  int* keys = reinterpret_cast<int*>(t.keys);
  int U = 0;
  for (int base0 = 0; base0 < T; base0 += WAVE) {
    const int i = base0 + lane_id();
    const uint32_t kt = t.keys[i];
    const unsigned long long lo = t.lo[i];
    const uint32_t hi = t.hi[i];
    const bool keep = kt != 0u && hi != Q_DROPPED;
    const double x = keep ? xs_to_double(hi, lo) : 0.0;
    const uint64_t m = __ballot(keep);
    wave_fence();
    if (keep) {
      const int pos = U + __popcll(m & lanemask_lt());
      vals[pos] = x;
      keys[pos] = (int)kt - 1;
    }
    wave_fence();
    U += __popcll(m);
  }
  if (U <= Kq) return U;
  const SelCrit c = select_top(U, Kq, [&](int i) { return keys[i]; }, [&](int i) { return vals[i]; }, hist, 0u,
                               TieIdAsc{});
  int U2 = 0;
  for (int i0 = 0; i0 < U; i0 += WAVE) {
    const int i = i0 + lane_id();
    const double x = i < U ? vals[i] : 0.0;
    const int k = i < U ? keys[i] : 0;
    const bool keep = i < U && sel_test(c, dbits(x), TieIdAsc{}(k, 0u));
    const uint64_t m = __ballot(keep);
    wave_fence();
    if (keep) { const int pos = U2 + __popcll(m & lanemask_lt()); vals[pos] = x; keys[pos] = k; }
    wave_fence();
    U2 += __popcll(m);
  }
  return U2 < Kq ? U2 : Kq;
}

__device__ __forceinline__ long long q_wave_sum64(long long x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(Q_WPB * WAVE) k_q_plan(DevSlab s, QArgs qa, int64_t nq, int wave_max, int T,
                                                          int32_t* code, int64_t* cand) {
  const int64_t q = (int64_t)blockIdx.x * Q_WPB + (threadIdx.x >> 6);
  if (q >= nq) return;
  const int l = lane_id();
  const int64_t sb = qa.qptr[q], se = qa.qptr[q + 1];
  long long C = 0, acc = 0;  // lane-partial candidates | candidates of key range l
  for (int64_t w0 = sb; w0 < se; w0 += WAVE) {
    const int64_t i = w0 + l;
    int len = 0;
    long long xr = 0;
    if (i < se) {
      const int u = qa.seeds[i];
      const int slot = res_slot(qa.part, qa.sA, qa.sB, u);
      len = res_len(s, slot, u);
      xr = s.xrow(slot, u);
    }
    C += len;
    const int nw = se - w0 < WAVE ? (int)(se - w0) : WAVE;
    for (int j = 0; j < nw; j++) {  // seed j of the window: 128 B of range index, lane l its range
      const int lj = __shfl(len, j);
      const long long xj = __shfl(xr, j);
      const int hi = l == NRANGE - 1 ? lj : min((int)s.rix[xj + l], lj);
      const int lo = l == 0 ? 0 : min((int)s.rix[xj + l - 1], lj);
      acc += hi > lo ? hi - lo : 0;
    }
  }
  C = q_wave_sum64(C);
  int verdict = Q_CODE_WIDE;
  if (wave_max > 0 && C <= (long long)wave_max) {  // (PPR_Q_WAVE_MAX=0: no query goes to the wave tier)
    int c = 0;
    while (c < Q_WAVE_CLASSES - 1 && 4 * C > 3ll * (Q_MIN_T << c)) c++;
    verdict = c;
  } else if (4 * C <= 3ll * T) {
    int lg = 8;
    while (4 * C > 3ll * (1 << lg)) lg++;
    verdict = Q_CODE_WG + lg;
  } else {
    const int v = acc < Q_SAT ? (int)acc : Q_SAT;
    const int incl = wave_incl_scan(v);
    const int lim = 3 * T / 4;
    for (int lg = 1; lg <= RANGE_BITS; lg++) {
      const int gs = NRANGE >> lg;  // ranges per group
      const int before = __shfl(incl, l >= gs ? l - gs : 0);
      const int sum = incl - (l >= gs ? before : 0);
      const bool over = (l % gs) == gs - 1 && sum > lim;
      if (!__ballot(over)) { verdict = Q_CODE_RANGE + lg; break; }
    }
  }
  if (l == 0) { code[q] = verdict; cand[q] = C; }
}

__global__ void __launch_bounds__(Q_WPB * WAVE) k_q_wave(DevSlab s, QArgs qa, const int32_t* list, int64_t count,
                                                          int T) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * Q_WPB + wv;
  if (w >= count) return;
  unsigned char* base = smem + (size_t)wv * q_wave_lds(T);
  const XTable t = xt_carve(base, T);
  uint32_t* hist = reinterpret_cast<uint32_t*>(base + xt_bytes(T));
  const int64_t q = list[w];
  const int64_t sb = qa.qptr[q], se = qa.qptr[q + 1];
  for (int i = lane_id(); i < T; i += WAVE) { t.keys[i] = 0u; t.lo[i] = 0ull; t.hi[i] = 0u; }
  wave_fence();
  const bool bad = q_accumulate(s, qa, sb, se, 0, NRANGE, t, 0, 1);
  wave_fence();
  if (__ballot(bad) && lane_id() == 0) probe_fail();
  if (qa.exclude) { q_exclude(t, qa, sb, se, lane_id(), WAVE); wave_fence(); }
  const int cnt = q_select(t, T, qa.Kq, hist);
  write_result_row(qa.out_ids, qa.out_sc, qa.out_len, q, qa.Kq, reinterpret_cast<uint64_t*>(t.lo),
                   reinterpret_cast<int*>(t.keys), cnt, T);
}

// shared body of k_q_wg / k_q_range: the whole workgroup clears and fills the table, wave 0
// selects. Returns the kept count in wave 0 (-1 in the other waves, which are done).
__device__ __forceinline__ int q_wg_merge(const DevSlab& s, const QArgs& qa, int64_t sb, int64_t se, int r0, int r1,
                                          const XTable& t, int T, uint32_t* hist) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < T; i += nthr) { t.keys[i] = 0u; t.lo[i] = 0ull; t.hi[i] = 0u; }
  __syncthreads();
  const bool bad = q_accumulate(s, qa, sb, se, r0, r1, t, tid >> 6, nthr >> 6);
  if (__ballot(bad) && lane_id() == 0) probe_fail();
  __syncthreads();
  if (qa.exclude) { q_exclude(t, qa, sb, se, tid, nthr); __syncthreads(); }
  if (tid >= WAVE) return -1;
  return q_select(t, T, qa.Kq, hist);
}

__global__ void __launch_bounds__(Q_WG_THREADS) k_q_wg(DevSlab s, QArgs qa, const int32_t* list, int T) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int64_t q = list[blockIdx.x];
  const XTable t = xt_carve(smem, T);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + xt_bytes(T));
  const int cnt = q_wg_merge(s, qa, qa.qptr[q], qa.qptr[q + 1], 0, NRANGE, t, T, hist);
  if (cnt < 0) return;
  write_result_row(qa.out_ids, qa.out_sc, qa.out_len, q, qa.Kq, reinterpret_cast<uint64_t*>(t.lo),
                   reinterpret_cast<int*>(t.keys), cnt, T);
}

__global__ void __launch_bounds__(Q_WG_THREADS) k_q_range(DevSlab s, QArgs qa, const QTask* tasks, int T, QLists ql) {
  extern __shared__ __align__(16) unsigned char smem[];
  const QTask tk = tasks[blockIdx.x];
  const XTable t = xt_carve(smem, T);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + xt_bytes(T));
  const int gs = NRANGE / tk.R;
  const int cnt = q_wg_merge(s, qa, qa.qptr[tk.q], qa.qptr[tk.q + 1], tk.g * gs, (tk.g + 1) * gs, t, T, hist);
  if (cnt <= 0) return;
  // append: the order of a list's entries is free (the final selection is by a total order)
  const double* vals = reinterpret_cast<const double*>(t.lo);
  const int* keys = reinterpret_cast<const int*>(t.keys);
  int pos = 0;
  if (lane_id() == 0) pos = atomicAdd(&ql.cnt[tk.rq], cnt);
  pos = __shfl(pos, 0);
  const int64_t o = ql.off[tk.rq], cap = ql.off[tk.rq + 1] - o;
  if ((int64_t)pos + cnt > cap) {  // (cannot happen: the list holds min(R Kq, C) entries)
    if (lane_id() == 0) probe_fail();
    return;
  }
  for (int i = lane_id(); i < cnt; i += WAVE) { ql.k[o + pos + i] = keys[i]; ql.v[o + pos + i] = vals[i]; }
}

__global__ void __launch_bounds__(WAVE) k_q_final(QArgs qa, const int32_t* rqq, QLists ql, int Kp) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint64_t* rv = reinterpret_cast<uint64_t*>(smem);
  int* rk = reinterpret_cast<int*>(smem + (size_t)Kp * 8);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + (size_t)Kp * 12);
  const int rq = blockIdx.x;
  const int64_t o = ql.off[rq], cap = ql.off[rq + 1] - o;
  const int n = ql.cnt[rq] < cap ? ql.cnt[rq] : (int)cap;
  const int32_t* lk = ql.k + o;
  const double* lv = ql.v + o;
  const int cnt = wave_select_compact(n, qa.Kq, [&](int i) { return lk[i]; }, [&](int i) { return lv[i]; }, hist,
                                      [&](int pos, int key, uint64_t vb) { rv[pos] = vb; rk[pos] = key; });
  wave_fence();
  write_result_row(qa.out_ids, qa.out_sc, qa.out_len, rqq[rq], qa.Kq, rv, rk, cnt, Kp);
}

}  // namespace pprk
