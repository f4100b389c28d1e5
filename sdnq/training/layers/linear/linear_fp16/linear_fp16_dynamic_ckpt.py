"""sdnq.training.layers.linear.linear_fp16.linear_fp16_dynamic_ckpt of the import-name drop-in: not built, the name raises NotImplementedError."""
from sdnq_amd.training import fp16_matmul_dynamic_with_backward_ckpt  # noqa: F401
