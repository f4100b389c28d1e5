"""sdnq.kernels.triton_atten of the import-name drop-in: ``sdnq_triton_atten`` is ``sdnq_amd.attention.sdnq_hip_atten``."""
from sdnq_amd.attention import sdnq_hip_atten as sdnq_triton_atten  # noqa: F401
