"""ConvTranspose1d / 2d / 3d forwards of SDNQ-quantized layers as GEMM + col2im.

Mirrors the reference's transposed-conv forwards (layers/conv/forward.py:85-99 ``quantized_conv_transpose_{1,2,3}d_forward``):
``F.conv_transposeNd(input, dequantize(W), bias, stride, padding, output_padding, groups, dilation)`` with ``output_padding`` from the
module's own ``_output_padding`` (so ``output_size=`` works as in torch).  The reference never runs these layers on a quantized matmul
(``use_quantized_matmul`` is forced off, quantizer.py:133), so there is one forward per dimensionality.

Computed here without the library convolution, like the conv forwards (conv.py):

    x [B, C_in, *in]  --ops.im2col, 1 x 1 kernel-->  x2d [B * L, C_in]                       (the channel-last activation operand)
    W (stored codes)  --ops.dequant_convt-------->   wd  [groups, P, C_in / groups]          (P = C_out / groups * prod(kernel))
    per conv group g: cols[:, g P : (g + 1) P] = x2d[:, g K' : (g + 1) K'] . wd[g]^T         (float GEMM, float32 store)
    cols [B * L, groups * P] --ops.col2im-------->   out [B, C_out, *out]                    (gather the taps, + bias, ONE rounding)

The columns of all groups side by side are exactly ``[C_out][prod(kernel)]`` in output-channel order, so one col2im launch serves any
``groups``.  Nothing synchronises with the host: the forward is stream-capturable.

Not built (``support.unsupported_reason`` names each): SVD factors, Hadamard rotation and codebooks on transposed convolutions, string /
non-zero padding modes, ``C_in / groups`` not a multiple of 16, ``P`` not a multiple of 16.
"""
from __future__ import annotations

import os

import torch

from . import linear, ops


class _State:
    """Kernel-ready tensors of one transposed-conv module, keyed like linear._State on the identity of its parameters."""
    __slots__ = ("key", "qw", "wd")


def _ntuple(v, n):
    return (int(v),) * n if isinstance(v, int) else tuple(int(e) for e in v)


def _state(mod) -> _State:
    st = mod.__dict__.get("_sdnq_hip_state")
    if st is not None:
        for name, ref, ptr, ver in st.key:
            t = linear._attr(mod, name)
            if t is not ref or (t is not None and (t.data_ptr() != ptr or linear._param_version(t) != ver)):
                break
        else:
            return st
    from .support import require
    require(mod)
    dq = mod.sdnq_dequantizer
    shape = tuple(int(d) for d in dq.original_shape)
    kprod = 1
    for d in shape[2:]:
        kprod *= d
    st = _State()
    st.key = linear._signature(mod)
    st.qw = ops.make_convt_weight(dq.weights_dtype, mod.weight, mod.scale, getattr(mod, "zero_point", None), shape[0], shape[1] * kprod, kprod)
    st.wd = None
    mod.__dict__["_sdnq_hip_state"] = st
    return st


def _forward(self, input: torch.Tensor, output_size, nd: int) -> torch.Tensor:
    dq = self.sdnq_dequantizer
    if input.ndim not in (nd + 1, nd + 2):
        raise RuntimeError(f"expected a {nd + 1}-D or {nd + 2}-D input to ConvTranspose{nd}d but got {input.ndim}-D")
    if input.dtype != dq.result_dtype:
        raise RuntimeError(f"expected input dtype {dq.result_dtype} (the layer's result_dtype) but got {input.dtype}")
    if not input.is_cuda:
        raise ops._lib.SdnqHipError("sdnq_amd forwards need CUDA/HIP tensors (no CPU fallback)")
    st = _state(self)
    stride, padding, dilation = _ntuple(self.stride, nd), _ntuple(self.padding, nd), _ntuple(self.dilation, nd)
    kernel = tuple(int(k) for k in dq.original_shape[2:])
    groups = int(self.groups)
    # forward.py:86 / :92 / :98 -- the module's own rule, including output_size=
    output_padding = self._output_padding(input, output_size, list(stride), list(padding), list(kernel), nd, list(dilation))
    batched = input.ndim == nd + 2
    x = input if batched else input.unsqueeze(0)
    b, c_in = int(x.shape[0]), int(x.shape[1])
    if c_in != int(dq.original_shape[0]):
        raise RuntimeError(f"expected {int(dq.original_shape[0])} input channels but got {c_in}")
    in_size = tuple(int(d) for d in x.shape[2:])
    out_size = tuple((in_size[i] - 1) * stride[i] - 2 * padding[i] + dilation[i] * (kernel[i] - 1) + int(output_padding[i]) + 1 for i in range(nd))
    c_out = int(dq.original_shape[1]) * groups
    if b == 0:
        return input.new_empty((0, c_out, *out_size))
    positions = 1
    for d in in_size:
        positions *= d
    kprod = 1
    for k in kernel:
        kprod *= k
    # channel-last activation operand [B * L, C_in]: the unfold kernel with a 1 x 1 window
    x2d, _ = ops.im2col(x.reshape(b, c_in, 1, positions), (1, 1), (1, 1), (0, 0), (1, 1))
    wd = st.wd
    if wd is None:
        wd = ops.dequant_convt(st.qw, dq.result_dtype, groups)  # [groups, P, C_in / groups]
        if linear.CACHE_WEIGHTS and os.environ.get("SDNQ_HIP_CACHE_DEQUANT", "0") == "1":  # as linear._float_forward keeps its operand
            st.wd = wd
    p_cols, kg = wd.shape[1], wd.shape[2]
    cols = torch.empty((b * positions, groups * p_cols), device=x.device, dtype=torch.float32)
    for g in range(groups):
        ops.linear_float_f32_into(x2d[:, g * kg:(g + 1) * kg], wd[g], cols, g * p_cols)
    out = ops.col2im(cols, linear._attr(self, "bias"), input.dtype, b, c_out, in_size, out_size, kernel, stride, padding, dilation)
    return out if batched else out.squeeze(0)


def _no_grad(fn):
    import functools

    @functools.wraps(fn)
    def forward(self, input, output_size=None):
        if torch.is_grad_enabled():
            with torch.no_grad():
                return fn(self, input, output_size)
        return fn(self, input, output_size)
    return forward


@_no_grad
def quantized_conv_transpose_1d_forward(self, input: torch.Tensor, output_size=None) -> torch.Tensor:
    return _forward(self, input, output_size, 1)


@_no_grad
def quantized_conv_transpose_2d_forward(self, input: torch.Tensor, output_size=None) -> torch.Tensor:
    return _forward(self, input, output_size, 2)


@_no_grad
def quantized_conv_transpose_3d_forward(self, input: torch.Tensor, output_size=None) -> torch.Tensor:
    return _forward(self, input, output_size, 3)
