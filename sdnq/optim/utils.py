"""sdnq.optim.utils of the import-name drop-in.  The reference's helpers here (get_param_grad, lerp_buffer_stochastic_, update_param_,
copy_stochastic_, apply_norm_to_update_) are the passes that ``sdnq_hip_adamw_step`` fuses into one launch; they have no separate form.
``QuantizedBuffer`` is what ``create_quantized_buffer`` makes there."""
from sdnq_amd.optim import QuantizedBuffer  # noqa: F401
