from pkg.modelling.metrics.index_recall import IndexRecall  # noqa: F401
from pkg.modelling.metrics.ranking_metrics import IndexRankingMetrics  # noqa: F401

__all__ = ["IndexRecall", "IndexRankingMetrics"]
