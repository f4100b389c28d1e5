"""sdnq.training.layers.linear.linear_int8.linear_int8_ckpt of the import-name drop-in: not built, the name raises NotImplementedError."""
from sdnq_amd.training import int8_matmul_with_backward_ckpt  # noqa: F401
