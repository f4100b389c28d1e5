"""Forward of quantized embedding layers (reference layers/embedding/forward.py:14-91): ``weight[ids]`` dequantized by ONE
gather-dequantize launch (``sdnq_hip_embedding``) that reads only the requested rows of the table.

Same contract as the reference's ``quantized_embedding_forward``: the rows come out in the layer's result dtype with the SVD
factors added and the Hadamard rotation applied, then multiplied by ``scalar_embed_scale`` when the layer has one
(``Gemma4TextScaledWordEmbedding``).  ``padding_idx`` rows are returned as stored and ``max_norm`` is ignored, as in the reference.
"""
from __future__ import annotations

import torch

from . import ops


def quantized_embedding_forward(self: torch.nn.Module, input: torch.Tensor) -> torch.Tensor:
    if not input.is_cuda:
        raise ops._lib.SdnqHipError("sdnq_amd forwards need CUDA/HIP tensors (no CPU fallback)")
    from .linear import _state  # the kernel-ready table descriptor, rebuilt when a parameter changes (support.require first)
    st = _state(self)
    dq = self.sdnq_dequantizer
    had = int(dq.hadamard_group_size) if dq.use_hadamard else 0
    return ops.embedding(st.qw, input, dq.result_dtype, had, getattr(self, "scalar_embed_scale", None))
