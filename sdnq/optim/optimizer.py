"""sdnq.optim.optimizer of the import-name drop-in: a view of ``sdnq_amd.optim``."""
from sdnq_amd.optim import SDNQOptimizer  # noqa: F401
