"""MI355X-native all-sources approximate Personalized PageRank (GRank / MCCompletePathV2).

Drop-in surface of fruttasecca/approximated_personalized_pagerank:
  * C++: include/ppr/grank.h, include/ppr/grankMulti.h (same templates, same signatures)
  * C ABI: include/ppr_hip.h (libppr_hip.so, built in-tree for gfx950)
  * Python: grank / grank_multi / GrankPlan (with GrankPlan.query: preference-set queries answered
    from the resident baskets, GrankPlan.rquery: the top sources of a target set, and GrankPlan.propagate / propagate_t / ppr.propagate:
    feature propagation through the table on the device, both ways, and GrankPlan.sweep / sweep_vectors: sweep-cut
    local clustering on the device, and GrankPlan.subgraphs: the subgraphs induced by each root's top PPR
    neighbours as one batched CSR / COO of device tensors, and GrankPlan.pairs / pair_scores: the scores,
    ranks and row overlaps of node pairs) / mccompletepathv2 / MccpPlan below, and the
    reference's quality harness (exact PPR, batched on the GPU; benchmark_algorithm).
"""
from ._lib import PprError
from .graph import Csr, import_edge_csv, read_edge_csv, rmat
from .grank import GrankPlan, GrankResult, PairResult, QueryResult, RQueryResult, SubgraphBatch, SweepResult, grank, grank_csr, grank_multi, normalize_pairs, propagate
from .mccp2 import MccpPlan, McStats, mccompletepathv2, mccp2_csr
from .exact import ExactPPR, benchmark_algorithm, jaccard, kendall_correlation

__all__ = [
    "PprError", "Csr", "rmat", "read_edge_csv", "import_edge_csv", "GrankPlan", "GrankResult", "QueryResult", "RQueryResult", "SweepResult", "SubgraphBatch", "PairResult", "normalize_pairs", "grank", "grank_csr",
    "grank_multi", "propagate", "MccpPlan", "McStats", "mccompletepathv2", "mccp2_csr", "ExactPPR", "benchmark_algorithm",
    "jaccard", "kendall_correlation",
]
