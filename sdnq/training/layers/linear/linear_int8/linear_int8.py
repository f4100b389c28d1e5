"""sdnq.training.layers.linear.linear_int8.linear_int8 of the import-name drop-in: not built, the name raises NotImplementedError."""
from sdnq_amd.training import int8_matmul_with_backward  # noqa: F401
