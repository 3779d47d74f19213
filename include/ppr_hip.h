/*
 * ppr_hip.h -- C ABI of the MI355X-native all-sources approximate PPR engine (libppr_hip.so).
 *
 * The reference (fruttasecca/approximated_personalized_pagerank) has no FFI: its surface is the
 * C++ templates ppr::grank / ppr::grankMulti / ppr::mccompletepathv2. This ABI is what those
 * templates bind to in the drop-in headers include/ppr/grank.h, include/ppr/grankMulti.h and
 * include/ppr/mccompletepathv2.h (same signatures as the reference), and what the Python mirror
 * binds with ctypes. Plain pointers and sizes only; no torch / HIP types in signatures
 * (streams are passed as void*).
 *
 * Dense ids: node i is the i-th key of the graph in its iteration order; col[] keeps each
 * node's successor order (the reference sums contributions in that order,
 * include/grank.h:107-116, and its partitions depend on the iteration order,
 * include/internal/pprInternal.h:57-63).
 *
 * All entry points are synchronous unless stated, thread-safe per call, and keep no globals.
 * Return value: PPR_OK (0) or a PPR_ERR_* code; ppr_strerror() names it.
 */
#ifndef PPR_HIP_H
#define PPR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PPR_OK = 0,
  PPR_ERR_ARG = 1,       /* bad pointer / size */
  PPR_ERR_K = 2,         /* "K must be positive"          include/grank.h:51 */
  PPR_ERR_L = 3,         /* "L must be positive"          include/grank.h:52 */
  PPR_ERR_KL = 4,        /* "K must be <= L"              include/grank.h:53 */
  PPR_ERR_ITERS = 5,     /* "iterations must be positive" include/grank.h:54 */
  PPR_ERR_DAMPING = 6,   /* "damping must be [0,1]"       include/grank.h:55 */
  PPR_ERR_THREADS = 7,   /* "nThreads must be positive"   header-only/grankMulti.h:304 */
  PPR_ERR_GRAPH = 8,     /* successor id out of range (UB in the reference, README.md:69-73) */
  PPR_ERR_HIP = 9,       /* HIP runtime failure (no device, launch failure, ...) */
  PPR_ERR_OOM = 10,      /* device allocation failed */
  PPR_ERR_RANGE = 11,    /* L / K / node count beyond what the kernels support */
  PPR_ERR_SOURCE = 12,   /* "source node not part of the graph" include/internal/pprSingleSource.h:39 */
  PPR_ERR_PROBE = 13     /* a bounded hash probe ran out of slots: a table sizing error (never on a
                            correct build; the exact-sum engines redo such a source instead) */
};

/* graph in dense CSR form (borrowed; host memory unless a *_dev entry point says otherwise) */
typedef struct ppr_csr {
  int64_t n;               /* nodes */
  const int64_t* row_ptr;  /* [n+1], row_ptr[0] = 0, edges m = row_ptr[n] */
  const int32_t* col;      /* [m] dense successor ids, successor order preserved */
} ppr_csr;

typedef struct ppr_opts {
  int32_t device;          /* HIP device ordinal; -1 = current device */
  int32_t flags;           /* PPR_FLAG_* */
  void* stream;            /* hipStream_t to run on; NULL = library-owned stream */
} ppr_opts;

enum {
  PPR_FLAG_STATS = 1,      /* collect candidate counts / algorithmic bytes per iteration */
  PPR_FLAG_CHAIN_SUM = 2   /* GRank: sum each key's contributions with the reference's in-order fma
                              chain (include/grank.h:107-116; bit-identical to it where no top-L tie
                              is cut). Default: the exact sum -- every contribution fl(s * d/deg)
                              added exactly, rounded once (order-free). The
                              environment variable PPR_SUM=chain|exact overrides the default. */
};

#define PPR_MAX_ITER_STATS 256

typedef struct ppr_stats {
  int32_t iterations_run;          /* iterations actually executed (tolerance may stop early) */
  int32_t reserved;
  double max_diff[PPR_MAX_ITER_STATS];   /* maxDiff of the partition updated in iteration i */
  double device_ms;                /* init + iterations + final top-K, device events */
  double merge_ms;                 /* basket-merge kernels only (sum over iterations) */
  int64_t candidates;              /* sum over iterations of candidates (PPR_FLAG_STATS) */
  int64_t algo_bytes;              /* SURVEY s8d algorithmic bytes over iterations (STATS) */
  int64_t merge_launches;          /* number of merge-kernel launches */
} ppr_stats;

const char* ppr_strerror(int code);

/* Build record of this library: "ppr_src_sha256=<hex> arch=<gfx target> hipcc=<clang version>".
 * The digest covers every source and header the library was compiled from (build.py); the Python
 * loader refuses a library whose digest differs from the sources beside it. No reference
 * counterpart (provenance of the drop-in binary). */
const char* ppr_build_info(void);

/* ---- host-side graph preparation (no GPU) ---- */

/* BFS 2-colouring of include/internal/pprInternal.h:29-99; part[i] = 0 for partitions.first */
int ppr_find_partitions_csr(const ppr_csr* g, uint8_t* part);
/* The same partitions computed on the device (`device` < 0: the current one): min-label components
 * and a level-synchronous BFS from each component's first node (csrc/partition.hip). Returns
 * PPR_ERR_RANGE for graphs that need more rounds than it allows (long paths): use the host BFS.
 * ppr_grank_plan_create / ppr_grank_csr take it when the caller passes no partitions, falling back
 * to the host BFS (PPR_HOST_BFS=1: the host BFS only). */
int ppr_find_partitions_csr_device(const ppr_csr* g, uint8_t* part, int32_t device);

/* MCCompletePathV2 node order, include/mccompletepathv2.h:36-113 (the same library sort on the
 * same records, so ties come out in the reference's order) */
int ppr_execution_order_csr(const ppr_csr* g, int32_t* order);

/* Edge-list importer of the reference CLI (src/main.cc:78-112): "a,b" per line, targets inserted
 * first, repeated edges kept once; dense ids follow the resulting unordered_map's iteration order
 * (the reference's). Call with keys/row_ptr/col NULL for n and m, then with buffers. */
int ppr_import_edge_csv(const char* path, int64_t* n, int64_t* m, int32_t* keys, int64_t* row_ptr,
                        int32_t* col);

/* Synthetic RMAT graph (Graph500 recursion, scrambled labels, deduped, successors ascending).
 * Call with col = NULL to get m (row_ptr[n+1] is filled either way); returns m or -error. */
int64_t ppr_rmat_generate(int32_t scale, int32_t edge_factor, double a, double b, double c,
                          uint64_t seed, int64_t* row_ptr, int32_t* col, int64_t col_cap);

/* ---- GRank (ppr::grank / ppr::grankMulti, include/grank.h:42-150) ----
 * One call: upload, init, iterate, final top-K, download. out_ids / out_scores are n*K
 * (row v = the K best (id, score) of source v, score desc, id asc; unused slots id -1),
 * out_len is n. part: partition bits from ppr_find_partitions_csr (or NULL to compute). */
int ppr_grank_csr(const ppr_csr* g, const uint8_t* part, uint32_t K, uint32_t L,
                  uint32_t iterations, double damping, double tolerance, const ppr_opts* o,
                  int32_t* out_ids, double* out_scores, int32_t* out_len, ppr_stats* st);

/* ---- device-resident plan (benchmarks, multi-GPU source sharding) ---- */
typedef struct ppr_plan ppr_plan;

/* Uploads the CSR and partition lists to HBM and allocates the two L-wide basket slabs. */
int ppr_grank_plan_create(const ppr_csr* g, const uint8_t* part, uint32_t K, uint32_t L,
                          double damping, const ppr_opts* o, ppr_plan** out);
void ppr_grank_plan_destroy(ppr_plan* p);

/* Whole device phase: init baskets, run up to `iterations` with the reference's stopping rule,
 * final top-K into the plan's device output. Inputs are already resident. */
int ppr_grank_plan_run(ppr_plan* p, uint32_t iterations, double tolerance, ppr_stats* st);

/* Step-level entry points (multi-GPU sharding; each is asynchronous on the plan's stream):
 *   init:    initial baskets of every node
 *   iterate: merge the active sources with index [begin, end) of iteration `it`'s active list
 *            (the partition's non-dangling nodes in dense-id order, see ppr_grank_plan_active_list), writing
 *            their new rows into the next-slot slab and folding norm1 into a device max
 *   finish:  final top-K of every node into the device output */
int ppr_grank_plan_init(ppr_plan* p);
int ppr_grank_plan_active_count(ppr_plan* p, int32_t it, int64_t* count);
int ppr_grank_plan_iterate(ppr_plan* p, int32_t it, int64_t begin, int64_t end);
int ppr_grank_plan_read_maxdiff(ppr_plan* p, int32_t it, double* maxdiff); /* syncs */
int ppr_grank_plan_finish(ppr_plan* p, int32_t iterations_run);

/* Row exchange for source sharding: pack/unpack of an active-list range of the rows iteration `it`
 * wrote, as one compact block: int64 off[cnt + 1] (payload offset per row, off[cnt] = payload
 * bytes), then per row int32 ids[Le] and f64 scores[len] (Le = len rounded up to even; a row
 * takes 12 len (+4 if len is odd) bytes, so len = (off[r+1] - off[r]) / 12). Only the entries
 * travel; the receiver rebuilds each row's minimum and hash-range index. Block size =
 * 8 (cnt + 1) + off[cnt] <= 8 + cnt * ppr_grank_plan_row_bytes; `cap` is the buffer's capacity.
 * Asynchronous on the plan's stream. */
int ppr_grank_plan_row_bytes(ppr_plan* p, int64_t* bytes);
int ppr_grank_plan_pack(ppr_plan* p, int32_t it, int64_t begin, int64_t end, void* dev_buf, int64_t cap);
int ppr_grank_plan_unpack(ppr_plan* p, int32_t it, int64_t begin, int64_t end, const void* dev_buf);
/* Active sources of iteration `it` in list order (host copy, nact entries), and the write-back of
 * an all-reduced maxDiff for a sharded iteration. */
int ppr_grank_plan_active_list(ppr_plan* p, int32_t it, int32_t* out);
int ppr_grank_plan_fold_maxdiff(ppr_plan* p, int32_t it, double maxdiff);

/* ---- source sharding over RCCL (one process per GPU) ----
 * Replaces the reference's per-iteration thread fan-out (header-only/grankMulti.h:376-396).
 * Rank 0 creates a 128-byte RCCL unique id, the caller broadcasts it (any channel), and every rank
 * calls ppr_grank_plan_comm_init. ppr_grank_plan_run_sharded then runs the whole job like
 * ppr_grank_plan_run, but each rank merges only its work-balanced range of every iteration's
 * active list (ppr_grank_plan_shard_bounds) and the rows it wrote travel as compact blocks on the
 * plan's stream:
 *   routed (default, up to 32 ranks): a row goes only to the ranks whose sources read it (its
 *     consumers, computed once per run from the CSR and the fixed bounds); per iteration one
 *     grouped ncclSend/ncclRecv of the exact 8-byte block sizes, then one of the blocks; after
 *     the last iteration each partition's final rows are broadcast once, so every rank ends with
 *     the whole slab;
 *   PPR_XROUTE=0: every rank's block to every rank (grouped ncclBroadcast at the block's bound,
 *     8 + rows * ppr_grank_plan_row_bytes, no size exchange).
 * maxDiff is combined with ncclAllReduce(MAX) on its IEEE bits, so every rank applies the
 * reference's stopping rule to the same value. Results equal the 1-GPU run bit for bit.
 * ppr_grank_plan_exchange_bytes: block bytes this rank received and rows it sent in its last
 * sharded run (no reference counterpart: measurement). */
int ppr_device_count(int32_t* count);
int ppr_comm_unique_id(void* id128);
int ppr_grank_plan_comm_init(ppr_plan* p, const void* id128, int32_t nranks, int32_t rank);
int ppr_grank_plan_shard_bounds(ppr_plan* p, int32_t it, int32_t nranks, int64_t* bounds);
int ppr_grank_plan_run_sharded(ppr_plan* p, uint32_t iterations, double tolerance, ppr_stats* st);
int ppr_grank_plan_exchange_bytes(ppr_plan* p, int64_t* recv_bytes, int64_t* rows_sent);
/* Measurement (no reference counterpart; tools/shard_floor.py): device milliseconds that rank
 * `rank` of a `world`-rank routed run spends in one of its sharded ends, timed on this one plan:
 * what 0 = its final top-K (own rows and the dangling ones; time it after a job), what 1 = its init
 * (own sources and the dangling nodes; rewrites those rows). */
int ppr_grank_plan_ends_time(ppr_plan* p, int32_t world, int32_t rank, int32_t iterations_run, int32_t what,
                             double* ms);
/* Per-kernel roofline of the last ppr_grank_plan_run (no reference counterpart: measurement).
 * Kernel groups, in this order: 0 wave tier (k_merge_lds_x), 1 sieve large (k_sv1 + k_svfin, 16
 * waves), 2 sieve mid (8 waves), 3 sieve small (4 waves), 4 sieve multi-slice (k_svA + k_svB +
 * k_svF), 5 range engines (k_xr + k_xfinal + k_xfin1: sources the sieve does not take or hands
 * back). bytes: SURVEY s8d algorithmic bytes of the sources the group merged (the wave tier's
 * without the written rows; the range group's with rows of min(L, candidates + 1) entries); ms:
 * HIP event time of the group's launches on its stream; launches:
 * event pairs summed. Up to n groups are written. */
int ppr_grank_plan_kernel_stats(ppr_plan* p, int32_t n, double* bytes, double* ms, int64_t* launches);
/* Tests: the same native loop with n plans of this process as the ranks (one thread each, block
 * exchange by device copies instead of RCCL: RCCL refuses two ranks on one GPU). st: n stats or
 * null. Every plan must be built on the same graph and parameters. */
int ppr_grank_plan_run_local_group(ppr_plan** plans, int32_t n, uint32_t iterations, double tolerance,
                                   ppr_stats* st);
/* host-staged variants of pack/unpack (rehearsal without RCCL; synchronous): pack_host writes the
 * block (at most cap bytes) and its size to *bytes; unpack_host takes a block of `bytes` bytes */
int ppr_grank_plan_pack_host(ppr_plan* p, int32_t it, int64_t begin, int64_t end, void* host_buf, int64_t cap,
                             int64_t* bytes);
int ppr_grank_plan_unpack_host(ppr_plan* p, int32_t it, int64_t begin, int64_t end, const void* host_buf,
                               int64_t bytes);

/* Downloads: final top-K (n*K) and the current L-slab (n*L, len per node; each row returned
 * sorted by (score desc, id asc) -- the device keeps rows in key-hash order). */
int ppr_grank_plan_fetch(ppr_plan* p, int32_t* out_ids, double* out_scores, int32_t* out_len);
int ppr_grank_plan_fetch_slab(ppr_plan* p, int32_t iterations_run, int32_t* ids, double* scores,
                              int32_t* len);
/* Rows [begin, end) of the final top-K (ids/scores (end - begin) * K, len end - begin; any may be
 * null), synchronous. With buffers from ppr_host_alloc (page-locked host memory: DMA at link rate
 * instead of a staged copy) the drop-in template downloads chunk by chunk while its threads
 * materialise the chunks already down (include/ppr/grank.h; no reference counterpart). */
int ppr_grank_plan_fetch_rows(ppr_plan* p, int64_t begin, int64_t end, int32_t* ids, double* scores,
                              int32_t* len);
int ppr_host_alloc(int64_t bytes, void** out);
void ppr_host_free(void* ptr);
/* Device stream the plan runs on (hipStream_t as void*), for event timing by the caller. Work the
 * plan puts on its internal side streams (hub bucket stage, wave tiers) is joined back into this
 * stream before each merge returns. */
void* ppr_grank_plan_stream(ppr_plan* p);
/* Raw basket slab slot (n*L ids / scores, n lengths; only the first len[v] entries of a row are
 * meaningful). MC plans: slot 0 = final baskets, slot 1 = random-walk baskets of the walk set. */
int ppr_plan_fetch_slot(ppr_plan* p, int32_t slot, int32_t* ids, double* scores, int32_t* len);

/* ---- preference-set queries from a plan's resident baskets ----
 * No reference counterpart: the reference returns the all-sources table and leaves its use to the
 * caller. By the linearity of PPR (Jeh & Widom) the vector personalised to a weighted set of
 * nodes is the weighted sum of the nodes' own vectors, PPR(sum_i f_i e_{u_i}) = sum_i f_i PPR(u_i),
 * and the plan holds those vectors in HBM: a query is one more basket merge, answered without
 * downloading the slab.
 * Q queries as a CSR: qptr[Q + 1] (qptr[0] = 0), seeds[qptr[Q]] (dense ids), weights[qptr[Q]] or
 * NULL (every weight 1.0). For query q with seeds u_i and weights w_i: W = w_0 + w_1 + ... summed
 * in seed order in fp64, f_i = w_i / W, and with B[u] the current L-wide basket of u after
 * `iterations_run` iterations (the slot rule of ppr_grank_plan_fetch_slab)
 *     total[k] = sum_i sum_{(k, s) in B[u_i]} floor(fl(s * f_i) * 2^93)
 * an exact integer sum; a key's score is total * 2^-93 rounded to nearest even once. Repeated
 * seeds add; a zero-weight seed contributes its keys with score 0 (zero scores are legal keys).
 * Row q of out_ids / out_scores (Q * Kq) holds the Kq best (id, score) by (score desc, dense id
 * asc) -- the same rule at the cut: a tie at the Kq-th place goes to the smaller id -- unused slots
 * id -1 / score 0; out_len[q] = min(Kq, distinct keys). PPR_QUERY_EXCLUDE_SEEDS removes the keys
 * that are seeds of the query (any weight) before the selection. A query without seeds gives an
 * empty row. The result depends only on the slab and the query, not on the engine that answered
 * it, the chunking of the call or the order of the queries.
 * Host pointers; synchronous on the plan's stream; writes nothing into the slabs or the plan's
 * top-K output, so a plan can be queried any number of times and run again afterwards.
 * Errors, all decided on the host before any merge kernel starts: PPR_ERR_ARG (null plan or
 * pointers, Q < 0, non-monotone qptr, a negative / NaN / infinite weight, a non-empty query whose
 * W is 0 or not finite, unknown flag bits, an MC plan), PPR_ERR_K (Kq = 0), PPR_ERR_RANGE
 * (Kq > 4096, or a query so wide that the candidates of one of its 64 key ranges exceed 3/4 of the
 * 8192-slot table: at most 393216 candidates = sum of len[seed] when they spread evenly),
 * PPR_ERR_SOURCE (a seed outside [0, n)).
 * MC plans are refused: their final scores are not bounded by 1 (the combine can reach
 * 1 / (1 - d)), so the 2^95 headroom of the 93-bit sums does not hold without a separate analysis. */
enum { PPR_QUERY_EXCLUDE_SEEDS = 1 };
typedef struct ppr_query_stats {
  double device_ms;            /* hipEvents on the plan's stream: upload excluded, kernels only */
  int64_t candidates;          /* sum of len[seed] over all seeds */
  int64_t algo_bytes;          /* per seed 4 + 4 + 12*len[seed]; per query 12*Kq + 4 */
  int64_t wave_queries, wg_queries, range_queries;   /* queries answered by each tier */
  int32_t max_ranges;          /* largest key-range split used (1..64) */
  int32_t reserved;
} ppr_query_stats;
int ppr_grank_plan_query(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* qptr,
                         const int32_t* seeds, const double* weights, uint32_t Kq, uint32_t flags,
                         int32_t* out_ids, double* out_scores, int32_t* out_len, ppr_query_stats* st);

/* ---- reverse queries: the top sources of a weighted target set ----
 * The other direction of the same resident table (no reference counterpart either): which sources
 * rank this item, or this weighted set of items, highest -- the matrix-vector product B f, a column
 * lookup in a table stored by rows, answered by scanning the rows' ids in HBM (or, for a handful of
 * targets, by probing every row through its range index) instead of downloading the slab.
 * Q queries as a CSR: qptr[Q + 1] (qptr[0] = 0), targets[qptr[Q]] (dense ids), weights[qptr[Q]] or
 * NULL (every weight 1.0). For query q with targets t_j and weights w_j: W = w_0 + w_1 + ... summed
 * in target order in fp64, f_j = w_j / W, and with B[u] the current L-wide basket of u after
 * `iterations_run` iterations (the slot rule of ppr_grank_plan_fetch_slab), for every source u
 *     X_q[u] = sum_j [t_j in B[u]] * floor(fl(B[u][t_j] * f_j) * 2^93)
 * an exact integer sum (one fp64 multiply per term); score(u) = X_q[u] * 2^-93 rounded to nearest
 * even once. Repeated targets add. A source is a hit of q when at least one target of q is a key of
 * B[u]; zero scores are legal (a zero-weight target still makes its sources hits). Every row sums
 * to <= 1 and sum f_j <= 1 + eps, so X < 2^95.
 * Row q of out_sources / out_scores (Q * Kq) holds the Kq best hits by (score desc, source id asc)
 * -- the same rule at the cut -- unused slots id -1 / score 0; out_len[q] = min(Kq, hits of q).
 * PPR_RQUERY_EXCLUDE_TARGETS drops the sources that are themselves targets of the query (any
 * weight) before the selection. A query without targets gives an empty row. The result depends
 * only on the slab and the query: not on the tier (scan or probe), the chunking, the batching of
 * the lists or the order of the queries.
 * Host pointers; synchronous on the plan's stream; writes nothing into the slabs or the plan's
 * top-K output.
 * Errors, all decided on the host before any kernel starts: PPR_ERR_ARG (null plan or pointers,
 * Q < 0, non-monotone qptr, a negative / NaN / infinite weight, a non-empty query whose W is 0 or
 * not finite, unknown flag bits, an MC plan -- for the forward query's reason), PPR_ERR_K (Kq = 0),
 * PPR_ERR_RANGE (Kq > 4096, or a single query with more targets than 3/4 of the 8192-slot target
 * table: 6144), PPR_ERR_SOURCE (a target outside [0, n)).
 * algo_bytes = the bytes the algorithm has to move: per pass over the slab's ids (scans)
 * 4 * sum len[u] + 4 * n; probe tier 4 per (row, posting) for the range-index pair + 4 per id of the
 * probed segments; per list entry (a hit source of a query) 8 for a score, 12 written and 12 read;
 * per query 12 * Kq + 4 for its result row. */
enum { PPR_RQUERY_EXCLUDE_TARGETS = 1 };
typedef struct ppr_rquery_stats {
  double device_ms;          /* HIP events around the kernels; uploads and downloads excluded */
  int64_t hits;              /* sum over queries of hit sources */
  int64_t algo_bytes;        /* see above */
  int64_t probe_queries, scan_queries;   /* queries answered by each tier */
  int64_t scans;             /* passes over the slab's ids (count and emit passes both counted) */
  int32_t chunks; int32_t reserved;
} ppr_rquery_stats;
int ppr_grank_plan_rquery(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* qptr,
                          const int32_t* targets, const double* weights, uint32_t Kq, uint32_t flags,
                          int32_t* out_sources, double* out_scores, int32_t* out_len, ppr_rquery_stats* st);

/* ---- feature propagation through the resident table, both ways ----
 * The dense products of the same table (no reference counterpart): Z = B[S] H, the PPRGo / APPNP
 * style aggregation of node features H [n, F] over the top-L PPR rows of a batch of S sources
 * (Bojchevski et al., "Scaling Graph Neural Networks with Approximate PageRank"), and its adjoint
 * Y = B[S]^T G for training through it. H / Z / G / Y are DEVICE pointers (everything else is host
 * memory): the table is not downloaded and the features are not staged through the host.
 * Common to both directions. GRank plans only. B[u] is the current row of u after `iterations_run`
 * iterations (the slot rule of ppr_grank_plan_fetch_slab; stored ids decoded to keys; the row
 * length clamped to [0, L]). Its entries (k_j, s_j), j = 0 .. len - 1, are taken in STORED ORDER,
 * ascending hash_b(k) (csrc/ppr_device.h): a function of the row's key set alone, not of the engine
 * that wrote the row. dt is PPR_PROP_F32 or PPR_PROP_BF16, shared by the input and the output of a
 * call; every sum is carried in fp64 and rounded to dt ONCE, to nearest even (bf16 straight from
 * the fp64 value, not through fp32). Weights w_j = s_j; with PPR_PROP_ROW_NORMALIZE
 * W = ((0.0 + s_0) + s_1) + ... in stored order with plain fp64 adds and w_j = s_j / W (one fp64
 * divide per entry), w_j = 0 when W == 0. sources: S dense ids (host), repeats allowed; NULL: S must
 * equal n and position i is source i.
 * Forward, ppr_grank_plan_propagate: H has n rows of F values with row stride ldh elements, Z has S
 * rows with stride ldz. For position i with u = sources[i] and every column c: acc = +0.0; for j in
 * stored order acc = fma(w_j, (double)H[k_j][c], acc) (an explicit fma); Z[i][c] = round_dt(acc).
 * A row of length 0 gives zeros.
 * Transposed, ppr_grank_plan_propagate_t: G has S rows with stride ldg, Y has n rows with stride
 * ldy; EVERY row of Y is written (a key no row of the batch holds gets zeros). The postings of key
 * k are all (i, w) such that k is a key of B[sources[i]], in ascending position i (keys are distinct
 * within a row: at most one posting per position). A key's list is cut into chunks of
 * PPR_PROP_CHUNK = 512 postings -- a constant of the contract; chunk m computes p_m = the fma chain
 * from +0.0 over its postings in order, acc = fma(w, (double)G[i][c], acc); the total is
 * ((p_0 + p_1) + p_2) ... with plain fp64 adds in chunk order; Y[k][c] = round_dt(total). No float
 * atomics are used: the result is bitwise reproducible.
 * Either result depends only on the slab and the arguments -- not on tiling, batching, knobs or the
 * order of anything -- and the calls write nothing into the slabs or the plan's top-K output.
 * Synchronous on the plan's stream (the caller synchronises the stream that produced H / G first).
 * Errors, all decided on the host before any kernel starts: PPR_ERR_ARG (null plan or pointers,
 * S < 0, NULL sources with S != n, a stride below F, F < 0, unknown dtype or flag bits, an MC plan),
 * PPR_ERR_RANGE (F == 0, F > 8192, or S > 2^30: positions are 32-bit), PPR_ERR_SOURCE (a source
 * outside [0, n)).
 * Stats: postings = sum of len over the positions (forward) / postings sorted (transposed);
 * algo_bytes = the bytes the algorithm has to move: per posting 12 (id and score) +
 * F * sizeof(dt) (the gathered feature row); per output row (S forward, n transposed)
 * F * sizeof(dt); per position 8. passes = key-range passes (1 forward), chunks = chunk tasks
 * (0 forward). ppr_grank_plan_device: the HIP device ordinal the plan lives on. */
enum { PPR_PROP_F32 = 0, PPR_PROP_BF16 = 1 };
enum { PPR_PROP_ROW_NORMALIZE = 1 };
#define PPR_PROP_CHUNK 512
typedef struct ppr_prop_stats {
  double device_ms;          /* HIP events around the kernels; uploads and downloads excluded */
  int64_t postings;
  int64_t algo_bytes;        /* see above */
  int64_t passes;
  int32_t chunks; int32_t reserved;
} ppr_prop_stats;
int ppr_grank_plan_propagate(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                             int32_t F, int32_t dt, uint32_t flags, const void* H, int64_t ldh, void* Z,
                             int64_t ldz, ppr_prop_stats* st);
int ppr_grank_plan_propagate_t(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                               int32_t F, int32_t dt, uint32_t flags, const void* G, int64_t ldg, void* Y,
                               int64_t ldy, ppr_prop_stats* st);
int ppr_grank_plan_device(ppr_plan* p, int32_t* device);

/* ---- sweep-cut local clustering from the resident table ----
 * The classic use of approximate PPR (no reference counterpart): local community detection by a
 * sweep cut (Andersen, Chung & Lang, "Local graph partitioning using PageRank vectors"). A seed's
 * PPR vector is swept in order of p[v] / deg(v); the prefix of lowest conductance is the seed's
 * community. The plan holds every node's vector and the graph in HBM, so the sweep of every requested
 * source is answered on the device, without downloading the slab.
 * The graph is taken as the plan stores it: directed, out-edges only, repeated edges with their
 * multiplicity (undirected clustering: pass a symmetric graph). deg(k) = row_ptr[k + 1] - row_ptr[k],
 * m = row_ptr[n]. Per source u, with B[u] its current row after `iterations_run` iterations (the slot
 * rule of ppr_grank_plan_fetch_slab; stored ids decoded to keys, undecodable ones skipped; the row
 * length clamped to [0, L]) and its entries (k, s):
 *   1. r = fl(s / (double)max(deg(k), 1)), one IEEE fp64 divide; the entries are sorted by (r
 *      descending, k ascending) and the first max_size are kept (max_size = 0: the row width L).
 *   2. Walking that order with vol += deg(k) in int64, the sweep stops BEFORE the first entry that
 *      would make vol > max_vol (max_vol = 0: floor(m / 2)). The `swept` entries before the stop are
 *      the sweep, with ranks 0 .. swept - 1; a source walks at most max_vol edges.
 *   3. For j = 1 .. swept: vol_j = sum of deg over the first j members; internal_j = the edges a -> b
 *      with both endpoints among the first j (self-loops count); cut_j = vol_j - internal_j;
 *      den_j = min(vol_j, m - vol_j); all int64.
 *   4. Among j in [min_size, swept] with den_j > 0 the smallest cut_j / den_j wins, compared exactly
 *      (cut_a den_b < cut_b den_a with 128-bit products), ties to the smaller j: out_size = j, out_cut,
 *      out_vol, out_phi = (double)cut / (double)den. With no admissible j (a dangling source's
 *      one-entry row, swept < min_size): size 0, cut = vol = 0, phi = +inf.
 * width = max_size ? max_size : L (vectors: max_size ? min(max_size, width_in) : width_in). Row i of
 * out_order (S * width) holds the swept members in order, then -1; out_swept[i] their number; row i
 * of prof_cut / prof_vol (S * width each, both or neither) holds cut_j / vol_j at j - 1, then -1.
 * sources: S dense ids, repeats allowed; NULL: S must equal n and position i is source i.
 * ppr_grank_plan_sweep_vectors sweeps R caller-supplied sparse vectors instead (a query's result
 * rows: the community of a seed set; an exact PPR top-K): rows of width_in (<= 4096) ids / scores, the
 * first lens[i] of row i meaningful, the same steps from 1 on.
 * The result depends only on the slab (or the vectors), the graph and the arguments: not on the tier
 * that answered a source, the slicing of its walk, the chunking, the knobs or the order of the sources.
 * Host pointers; synchronous on the plan's stream; writes nothing into the slabs or the top-K output.
 * Errors, all decided on the host before any kernel starts: PPR_ERR_ARG (null plan or pointers, S < 0,
 * NULL sources with S != n, min_size = 0 or > width, max_vol < 0 or > m, only one of the two profile
 * pointers, unknown flag bits -- none is defined --, an MC plan; vectors: a length outside
 * [0, width_in], a negative / NaN / infinite score, a repeated id within a row), PPR_ERR_RANGE
 * (max_size > 4096 or width_in > 4096), PPR_ERR_SOURCE (a source or id outside [0, n)).
 * algo_bytes = the bytes the algorithm has to move: per row entry 28 (id 4, score 8, the two row
 * pointer words of its degree 16); per walked edge 4; per source 4 * width + 36 (its order and the
 * five result words), plus 16 * width with profiles. */
typedef struct ppr_sweep_stats {
  double device_ms;          /* HIP events around the kernels; uploads and downloads excluded */
  int64_t edges;             /* edges walked = sum of vol_swept over the sources */
  int64_t algo_bytes;        /* see above */
  int64_t wave_sources, wg_sources, slice_sources;   /* sources answered by each tier */
  int32_t chunks; int32_t reserved;
} ppr_sweep_stats;
int ppr_grank_plan_sweep(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                         uint32_t min_size, uint32_t max_size, int64_t max_vol, uint32_t flags,
                         int32_t* out_order, int32_t* out_swept, int32_t* out_size, int64_t* out_cut,
                         int64_t* out_vol, double* out_phi, int64_t* prof_cut, int64_t* prof_vol,
                         ppr_sweep_stats* st);
int ppr_grank_plan_sweep_vectors(ppr_plan* p, int64_t R, int32_t width_in, const int32_t* ids,
                                 const double* scores, const int32_t* lens, uint32_t min_size,
                                 uint32_t max_size, int64_t max_vol, uint32_t flags, int32_t* out_order,
                                 int32_t* out_swept, int32_t* out_size, int64_t* out_cut, int64_t* out_vol,
                                 double* out_phi, int64_t* prof_cut, int64_t* prof_vol, ppr_sweep_stats* st);

/* ---- PPR-induced subgraph batches from the resident table ----
 * Subgraph sampling by PPR for GNN minibatches (no reference counterpart): for each root of a batch
 * its top PPR neighbours and the subgraph they induce (ShaDow-GNN, Zeng et al., "Decoupling the Depth
 * and Scope of Graph Neural Networks"; GraphSAINT's and PPRGo's PPR samplers), as one batched CSR /
 * COO in DEVICE memory, without downloading the slab.
 * The graph is taken as the plan stores it: directed, out-edges only, repeated edges with their
 * multiplicity, self-loops kept, bit 31 of a stored target masked off; deg(k) = row_ptr[k + 1] -
 * row_ptr[k]. GRank plans only. sources: S dense ids (host), repeats allowed; NULL: S must equal n
 * and position i is source i.
 * Members. For position i with u = sources[i]:
 *   1. B[u] is the current row of u after `iterations_run` iterations (the slot rule of
 *      ppr_grank_plan_fetch_slab; stored ids decoded to keys, undecodable ones skipped; the row
 *      length clamped to [0, L]).
 *   2. Its entries are ordered by (score descending, key ascending); scores are >= +0, so their bit
 *      patterns order like the values.
 *   3. With PPR_SUBG_ROOT_FIRST the entry whose key is u moves to the front, the others keep their
 *      order (a GRank row always holds it; were it absent, the flag has no effect for that position).
 *   4. The first `size` entries are kept (size = 0: the row width L): the c_i = min(size, decodable
 *      length) members of position i, with ranks 0 .. c_i - 1.
 * Edges. A member a with max_deg > 0 and deg(a) > max_deg emits no out-edges (it stays a node and
 * still receives edges; max_deg = 0: no cap). Every other member a emits one edge per position p of
 * its adjacency list whose target col[p] & 0x7fffffff is a member of the same position. The edges of
 * the batch are ordered by (position i, rank of a, p) ascending: the graph's own order, filtered.
 * Outputs, with N = sum c_i and E = all edges; node_ptr / edge_ptr are HOST arrays, the others
 * DEVICE pointers:
 *   node_ptr[S + 1], edge_ptr[S + 1]  int64, exclusive prefix sums of c_i / of the edges per position
 *   nodes[N]       global keys: member j of position i at node_ptr[i] + j, which is its batch id
 *   scores[N]      fp64, optional (NULL: not written): the row's score of each member, bit for bit
 *   rowptr[N + 1]  rowptr[node_ptr[i] + j] = edge_ptr[i] + edges emitted by the members of position i
 *                  before j; rowptr[N] = E
 *   col[E]         batch id of the target
 *   row[E]         optional: batch id of the emitting member (COO)
 *   eid[E]         int64, optional: the position p in the plan's edge array
 * nodes, rowptr, col and row share one index type: int32, or int64 with PPR_SUBG_IDX64.
 * The result depends only on the slab, the graph and the arguments: not on the tier that answered a
 * source, the slicing of its walk, the chunking, the knobs or the order of the sources (a position's
 * rows are the same up to its node_ptr / edge_ptr offsets wherever it stands). No float atomics; no
 * output position is decided by the arrival order of atomics (the edges are counted per 64-edge
 * group of a fixed numbering of the walk, the counts are scanned, and the second pass writes every
 * hit at its group's offset plus its lane's rank among the group's hits). Synchronous on the plan's
 * stream (the caller synchronises the stream that produced the output tensors first); writes nothing
 * into the slabs or the plan's top-K output.
 * Capacities. node_cap / edge_cap are the element capacities of the device arrays: nodes and scores
 * hold node_cap elements, rowptr node_cap + 1, col / row / eid edge_cap. A COUNT-ONLY call has every
 * device pointer NULL and both capacities 0: node_ptr / edge_ptr are filled, PPR_OK. When N > node_cap
 * or E > edge_cap the call returns PPR_ERR_RANGE with node_ptr / edge_ptr complete and valid (the
 * caller allocates from them); the contents of the device arrays are then unspecified, and nothing is
 * written at or beyond index node_cap of nodes / scores / rowptr or edge_cap of col / row / eid.
 * N or E above 2^31 - 1 without PPR_SUBG_IDX64: PPR_ERR_RANGE as well, host arrays complete.
 * A source whose uncapped members have more than 2^30 out-edges in total: PPR_ERR_RANGE (set max_deg).
 * Refusals, all decided on the host before any kernel starts, in this order; they leave every output
 * untouched (st is cleared): PPR_ERR_ARG (null plan, an MC plan, iterations_run < 0, null node_ptr or
 * edge_ptr, S < 0; then NULL sources with S != n; then unknown flag bits; then max_deg < 0 or a
 * negative capacity; then some but not all of nodes / rowptr / col NULL; then all three NULL with an
 * optional pointer or a capacity given), PPR_ERR_RANGE (size > 4096 or S > 2^30), PPR_ERR_SOURCE (a
 * source outside [0, n)).
 * Stats: edges_walked = sum of deg over the uncapped members; capped_members = members that max_deg
 * silenced; algo_bytes = the bytes the algorithm has to move, with X the index size (4 or 8): per
 * decodable row entry 12 (id and score); per member 16 (the two row pointer words of its degree)
 * and, unless count-only, 2 X (nodes, rowptr) + 8 with scores; per walked edge 4 in the count pass
 * and 4 more when the emit pass ran; per 64-edge group 8 (its count written, its offset read); per
 * emitted edge X, + X with row, + 8 with eid. */
enum { PPR_SUBG_ROOT_FIRST = 1, PPR_SUBG_IDX64 = 2 };
typedef struct ppr_subg_stats {
  double device_ms;          /* HIP events around the kernels; uploads and downloads excluded */
  int64_t edges_walked;
  int64_t edges, nodes;      /* E, N */
  int64_t capped_members;
  int64_t algo_bytes;        /* see above */
  int64_t wave_sources, wg_sources, slice_sources;   /* sources answered by each tier */
  int32_t chunks; int32_t reserved;
} ppr_subg_stats;
int ppr_grank_plan_subgraphs(ppr_plan* p, int32_t iterations_run, int64_t S, const int32_t* sources,
                             uint32_t size, int64_t max_deg, uint32_t flags, int64_t node_cap,
                             int64_t edge_cap, int64_t* node_ptr, int64_t* edge_ptr, void* nodes,
                             double* scores, void* rowptr, void* col, void* row, int64_t* eid,
                             ppr_subg_stats* st);

/* ---- node-pair scores from the resident table ----
 * The most basic question about the table (no reference counterpart): what is B[u][v], and how
 * similar are the rows of u and v? The PPR score of a pair is the standard link-prediction feature
 * and Hits@K / MRR need the rank of a target inside the source's row; candidate re-ranking needs the
 * forward score, the backward score and the row overlap; node similarity the Jaccard or cosine of two
 * rows. Answered on the device, without downloading the slab. GRank plans only.
 * Q groups as a CSR: gptr[Q + 1] (gptr[0] = 0), sources[Q], cands[P] with P = gptr[Q]; group q scores
 * its source u = sources[q] against each candidate v = cands[j], j in [gptr[q], gptr[q + 1]). Repeated
 * sources, repeated candidates, v == u and groups without candidates are legal.
 * B[x] is the current row of x after `iterations_run` iterations (the slot rule of
 * ppr_grank_plan_fetch_slab; stored ids decoded to keys, undecodable ones skipped; the row length
 * clamped to [0, L]); len(x) = its decodable entries.
 * Outputs, each indexed by the candidate position j except out_slen (by q); each is optional: NULL =
 * not computed and not written.
 *   out_fwd[j]     the score of key v in B[u], bit for bit, +0.0 when v is absent
 *   out_bwd[j]     the score of key u in B[v], bit for bit, +0.0 when u is absent
 *   out_hit[j]     bit 0: v is a key of B[u]; bit 1: u is a key of B[v] (zero scores are legal keys,
 *                  so a score cannot tell absent from zero)
 *   out_rank[j]    the 0-based position of v among the decodable entries of B[u] ordered by (score
 *                  descending, key ascending), -1 when v is absent (scores are >= +0, so their bit
 *                  patterns order like the values)
 *   out_common[j]  |keys(B[u]) & keys(B[v])|
 *   out_dot[j]     over the common keys k, X = sum floor(fl(B[u][k] * B[v][k]) * 2^93), each term one
 *                  fp64 multiply, the sum an exact integer; the result is X * 2^-93 rounded to nearest
 *                  even once. The sum has no order: dot(u, v) and dot(v, u) have the same bits. Every
 *                  GRank row sums to <= 1 (the bound ppr_grank_plan_rquery states), so the products sum
 *                  to <= 1 and X < 2^95 fits the 96-bit sum. An MC plan's scores are not bounded by 1
 *                  (its totals reach deg / d), so the sum could overflow: MC plans are refused.
 *   out_slen[q] = len(u), out_clen[j] = len(v): with out_common they give the Jaccard, with
 *                  dot(u, u) and dot(v, v) the cosine.
 * Two work classes, chosen per call: with out_common and out_dot both NULL (lookup class) no row is
 * walked for a pair -- v is searched in the one 1/64 segment of B[u] its hash range names, u in B[v] the
 * same way; otherwise (overlap class) B[u] is held in LDS per group task and the candidates' rows are
 * streamed against it. The result depends only on the slab and the arguments: not on the class, the
 * tier, how groups were split or chunked, the knobs or the order of groups or candidates. No float
 * atomics; every output position is fixed by j alone.
 * Host pointers; synchronous on the plan's stream; writes nothing into the slabs or the plan's top-K
 * output.
 * Refusals, all decided on the host before any kernel starts, in this order; they leave every output
 * untouched (st is cleared): PPR_ERR_ARG (a null plan, an MC plan, iterations_run < 0, null gptr,
 * Q < 0; then gptr[0] != 0 or a decreasing gptr; then null sources with Q > 0; then null cands with
 * P > 0; then unknown flag bits -- none is defined; then every output pointer NULL), PPR_ERR_RANGE (Q or
 * P above 2^31 - 1), PPR_ERR_SOURCE (a source or candidate outside [0, n)). A call with Q == 0, or with
 * P == 0 and no out_slen, returns PPR_OK without a launch.
 * Stats: pairs = P, groups = Q, lookup_pairs + overlap_pairs = P (the class of the call),
 * entries_read = row ids the kernels read; wave_groups / wg_groups / split_groups = the groups of an
 * overlap-class call by tier (every group has exactly one; all 0 in the lookup class).
 * algo_bytes = the bytes the algorithm has to move, with len the stored length of a row. Both classes:
 * per pair the requested outputs (fwd 8, bwd 8, hit 1, rank 4, common 4, dot 8, clen 4) + 4 for the
 * candidate id; per group 4 for the source id and, with out_slen, 4 + 4 len(u) (the ids are decoded to
 * be counted). Overlap class: per group task 12 len(u) + 128 for the row and its range index, + 2 len(u)
 * with out_rank; per pair 4 len(v) for the ids, + 8 common for the scores of the hits with out_dot.
 * Lookup class: per pair 8 for the two range-index reads + 4 for the pair's group index + 4 per id of
 * the two probed segments + 8 per hit score, + 4 len(v) with out_clen; with out_rank 14 len(u) + 128
 * once per group (ids, scores, the range index, the 2-byte ranks written) and 2 per forward hit. */
typedef struct ppr_pairs_stats {
  double device_ms;          /* HIP events around the kernels; uploads and downloads excluded */
  int64_t pairs, groups;
  int64_t lookup_pairs, overlap_pairs;
  int64_t entries_read;
  int64_t algo_bytes;        /* see above */
  int64_t wave_groups, wg_groups, split_groups;
  int32_t chunks; int32_t reserved;
} ppr_pairs_stats;
int ppr_grank_plan_pairs(ppr_plan* p, int32_t iterations_run, int64_t Q, const int64_t* gptr,
                         const int32_t* sources, const int32_t* cands, uint32_t flags,
                         double* out_fwd, double* out_bwd, uint8_t* out_hit, int32_t* out_rank,
                         int32_t* out_common, double* out_dot, int32_t* out_slen, int32_t* out_clen,
                         ppr_pairs_stats* st);

/* ---- MCCompletePathV2 (ppr::mccompletepathv2, include/mccompletepathv2.h:182-258) ----
 * `walks` is the reference's `iterations` (R): floor(R*d) walks per walk-set node. The walks use
 * counter-based Philox4x32-10 keyed by `seed` (the reference seeds a global mt19937 from
 * std::random_device, so runs are only statistically comparable); the combine is deterministic.
 * Results: out_ids / out_scores n*K (rows score desc, id asc, unused id -1), out_len n. */
typedef struct ppr_mc_stats {
  double device_ms;        /* walks + combine + top-K, device events */
  double walk_ms;          /* k_mc_walk */
  double combine_ms;       /* level-synchronous merge kernels */
  int64_t walk_nodes;      /* |W|: nodes whose random-walk basket some predecessor reads */
  int64_t walks;           /* walks run (|W| * floor(R*d)) */
  int64_t levels;          /* combine levels */
  int64_t merge_launches;
  int64_t candidates;      /* combine candidates (PPR_FLAG_STATS) */
  int64_t algo_bytes;      /* combine algorithmic bytes (PPR_FLAG_STATS) */
} ppr_mc_stats;

int ppr_mccp2_csr(const ppr_csr* g, uint32_t K, uint32_t L, uint32_t walks, double damping,
                  uint64_t seed, const ppr_opts* o, int32_t* out_ids, double* out_scores,
                  int32_t* out_len, ppr_mc_stats* st);
/* Plan form: executionOrder, walk set and combine levels are computed once and the graph stays
 * resident. ppr_mccp2_plan_walk runs the walks of walk-set entries [begin, end) (walk-count
 * sharding across GPUs needs no exchange); combine merges level by level and writes the top-K,
 * fetched with ppr_grank_plan_fetch; destroy with ppr_grank_plan_destroy. */
int ppr_mccp2_plan_create(const ppr_csr* g, uint32_t K, uint32_t L, double damping,
                          const ppr_opts* o, ppr_plan** out);
int ppr_mccp2_plan_info(ppr_plan* p, int64_t* walk_nodes, int64_t* levels, int64_t* dangling);
int ppr_mccp2_plan_walk(ppr_plan* p, uint32_t walks, uint64_t seed, int64_t begin, int64_t end);
int ppr_mccp2_plan_combine(ppr_plan* p);
int ppr_mccp2_plan_run(ppr_plan* p, uint32_t walks, uint64_t seed, ppr_mc_stats* st);
/* The whole MC job on several ranks (one process per GPU, after ppr_grank_plan_comm_init on the MC
 * plan): each rank walks an equal contiguous range of the walk set, the walk baskets are
 * all-gathered as compact blocks (exact sizes all-gathered and checked first, then one grouped
 * ncclBroadcast per rank), and every rank runs the level-sequential combine and the top-K. The
 * result equals ppr_mccp2_plan_run with the same seed bit for bit on every rank. st: walk_ms and
 * walks are this rank's share; ppr_grank_plan_exchange_bytes gives the walk-basket bytes it
 * received. (Replaces the single-process sweep of include/mccompletepathv2.h:211-250.) */
int ppr_mccp2_plan_run_sharded(ppr_plan* p, uint32_t walks, uint64_t seed, ppr_mc_stats* st);
/* Tests: the same with n MC plans of this process as the ranks (device copies instead of RCCL). */
int ppr_mccp2_plan_run_local_group(ppr_plan** plans, int32_t n, uint32_t walks, uint64_t seed,
                                   ppr_mc_stats* st);

/* ---- Exact single-source PPR, batched (the reference's quality oracle) -------------------------
 * Replaces ppr::pprInternal::pprSingleSource(graph, iterations, damping, tolerance, source)
 * (include/internal/pprSingleSource.h:28-75) for S sources at once, and the keepTop(K) +
 * score lookups benchmarkAlgorithm does on its result (include/benchmarkAlgorithm.h:91-121).
 * Scores agree with the reference to rounding (the per-node summation order differs). */
typedef struct ppr_exact ppr_exact;
int ppr_exact_create(const ppr_csr* g, const int32_t* sources, int32_t S, double damping,
                     const ppr_opts* o, ppr_exact** out);
/* power iteration of every source until its norm1 step < tolerance or `iterations`;
 * iters_run[S] (optional): iterations each source ran */
int ppr_exact_run(ppr_exact* h, uint32_t iterations, double tolerance, int32_t* iters_run);
/* keepTop(K) of every source's vector (nonzero entries), rows [S][K] by (score desc, id asc) */
int ppr_exact_topk(ppr_exact* h, uint32_t K, int32_t* out_ids, double* out_scores, int32_t* out_len);
/* out[s][q] = score of node keys[s][q] for source s (0 for a node it never reached) */
int ppr_exact_gather(ppr_exact* h, int32_t Q, const int32_t* keys, double* out);
void ppr_exact_destroy(ppr_exact* h);

#ifdef __cplusplus
}
#endif
#endif /* PPR_HIP_H */
