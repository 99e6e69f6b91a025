"""Stage-2 evaluation (the reference's `evaluate` package): retrieval metrics of generated semantic ids."""
from .metrics import NDCGAccumulator, RetrievalMetrics, TopKAccumulator, actual_with_tags  # noqa: F401
