"""sdnq.kernels.triton_atten_backward of the import-name drop-in: ``sdnq_triton_atten_with_backward`` is
``sdnq_amd.attention.sdnq_hip_atten_with_backward``."""
from sdnq_amd.attention import sdnq_hip_atten_with_backward as sdnq_triton_atten_with_backward  # noqa: F401
