"""sdnq.optim.adamw of the import-name drop-in: a view of ``sdnq_amd.optim``."""
from sdnq_amd.optim import AdamW, SDNQOptimizer  # noqa: F401
