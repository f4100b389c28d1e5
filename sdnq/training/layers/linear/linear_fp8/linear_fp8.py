"""sdnq.training.layers.linear.linear_fp8.linear_fp8 of the import-name drop-in: not built, the name raises NotImplementedError."""
from sdnq_amd.training import fp8_matmul_with_backward  # noqa: F401
