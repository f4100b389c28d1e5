"""sdnq.training.layers.linear.linear_fp16.linear_fp16 of the import-name drop-in: not built, the name raises NotImplementedError."""
from sdnq_amd.training import fp16_matmul_with_backward  # noqa: F401
