"""sdnq.training.layers.linear.linear_uint8.linear_uint8 of the import-name drop-in: not built, the name raises NotImplementedError."""
from sdnq_amd.training import uint8_matmul_with_backward  # noqa: F401
