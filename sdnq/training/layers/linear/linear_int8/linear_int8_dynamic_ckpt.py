"""sdnq.training.layers.linear.linear_int8.linear_int8_dynamic_ckpt of the import-name drop-in: views of ``sdnq_amd.training``."""
from sdnq_amd.training import (  # noqa: F401
    INT8MatmulDynamicBackwardCKPT,
    int8_matmul_dynamic_with_backward_ckpt,
    quantized_linear_forward_int8_matmul_dynamic_ckpt,
)
