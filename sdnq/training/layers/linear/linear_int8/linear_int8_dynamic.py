"""sdnq.training.layers.linear.linear_int8.linear_int8_dynamic of the import-name drop-in: views of ``sdnq_amd.training``."""
from sdnq_amd.training import (  # noqa: F401
    INT8MatmulDynamicBackward,
    int8_matmul_dynamic,
    int8_matmul_dynamic_with_backward,
    quantized_linear_forward_int8_matmul_dynamic,
)
