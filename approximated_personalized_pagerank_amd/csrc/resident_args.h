// resident_args.h -- what a call answered from a plan's resident baskets (query.hip, rquery.hip,
// propagate.hip) decides on the host before it touches the device: the refusals of a weighted CSR of
// id sets and its factors, the id-range check, the slot rule and the power of two that holds Kq.
// Pure host code, no HIP: tests/cpp/resident_args_test.cpp includes only this header.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ppr_hip.h"
#include "hash32.h"

namespace pprres {

// slab slot that holds the current row of a partition-0 (sA) / partition-1 (sB) node after
// `iterations_run` iterations: the partitions are updated in turn, each into its other slot
struct SlotPair {
  int sA, sB;
};
inline SlotPair slot_pair(int32_t iterations_run) {
  return SlotPair{((iterations_run + 1) / 2) & 1, (iterations_run / 2) & 1};
}

// Kp: the smallest power of two >= Kq (the LDS room of a result row)
inline int pow2_at_least_k(uint32_t Kq) {
  int Kp = 1;
  while (Kp < (int)Kq) Kp <<= 1;
  return Kp;
}

// every id in [0, n), else PPR_ERR_SOURCE
inline int check_ids(const int32_t* ids, int64_t count, int64_t n) {
  for (int64_t i = 0; i < count; i++)
    if (ids[i] < 0 || (int64_t)ids[i] >= n) return PPR_ERR_SOURCE;
  return PPR_OK;
}

// The refusals of Q weighted id sets in CSR form (qptr, ids, weights; null weights: all 1) and the
// factors f_i = w_i / W, W summed in set order in fp64. `call_ok`: the plan serves such calls and
// iterations_run >= 0; `outs_ok`: the three output pointers are there. The order of the checks is
// part of the contract: a call that is wrong in two ways gets the code of the first one below.
inline int check_weighted_sets(bool call_ok, int64_t n, int64_t Q, const int64_t* qptr, const int32_t* ids,
                               const double* weights, bool outs_ok, uint32_t Kq, uint32_t max_k, uint32_t flags,
                               uint32_t allowed_flags, std::vector<double>& fac) {
  if (!call_ok || Q < 0 || !qptr) return PPR_ERR_ARG;
  if (Q > 0 && !outs_ok) return PPR_ERR_ARG;
  if (flags & ~allowed_flags) return PPR_ERR_ARG;
  if (Kq == 0) return PPR_ERR_K;
  if (Kq > max_k) return PPR_ERR_RANGE;
  if (qptr[0] != 0) return PPR_ERR_ARG;
  for (int64_t q = 0; q < Q; q++)
    if (qptr[q + 1] < qptr[q]) return PPR_ERR_ARG;
  const int64_t N = qptr[Q];
  if (N > 0 && !ids) return PPR_ERR_ARG;
  if (check_ids(ids, N, n)) return PPR_ERR_SOURCE;
  fac.assign((size_t)(N > 1 ? N : 1), 0.0);
  for (int64_t q = 0; q < Q; q++) {
    const int64_t b = qptr[q], e = qptr[q + 1];
    double W = 0.0;
    for (int64_t i = b; i < e; i++) {
      const double w = weights ? weights[i] : 1.0;
      if (!(w >= 0.0) || !std::isfinite(w)) return PPR_ERR_ARG;  // negative, NaN, infinite
      W += w;  // in set order
    }
    if (e > b && (!(W > 0.0) || !std::isfinite(W))) return PPR_ERR_ARG;
    for (int64_t i = b; i < e; i++) fac[i] = (weights ? weights[i] : 1.0) / W;
  }
  return PPR_OK;
}

}  // namespace pprres
