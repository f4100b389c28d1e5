"""The int8 training Linear of the reference (training/layers/linear/linear_int8/linear_int8_dynamic.py and linear_int8_dynamic_ckpt.py) on
HIP kernels: three int8 matmuls per layer call -- y, grad_input, grad_weight -- whose operands are quantized on the fly from float tensors.

    y           = scaled_mm(rowquant(x)  [M][K], rowquant(W)     [N][K])      + bias
    grad_input  = scaled_mm(rowquant(dY) [M][N], colquant_t(W)   [K][N])      one scale per input channel k (quantize_int_mm(W, dim=0))
    grad_weight = scaled_mm(colquant_t(dY) [N][M'], colquant_t(x) [K][M'])    both operands quantized along the token axis; M' = M
                                                                              rounded up to 16, the pad columns are zero codes
    grad_bias   = colsum(dY)                                                  out of the same pass that quantizes dY per column

``ops.rowquant`` quantizes along the contiguous axis, ``ops.colquant_t`` (csrc/colquant.hip) along the other one and hands the codes
over transposed, so all three products run on the one int8 GEMM (``ops.scaled_mm``).  The ckpt form quantizes W and x per column inside
the forward and saves only those int8 codes and float32 scales; its results are bit-identical to the plain form's.

Built: plain float weights (float32 / bfloat16 / float16), N % 16 == 0 and K % 16 == 0.  Everything else the reference's training
package offers raises NotImplementedError naming the configuration; there is no float fallback except the reference's own rule for fewer
than 32 rows (linear_int8_dynamic.py:209-215).  Nothing here synchronises with the host: a forward + backward can be stream-captured.
"""
from __future__ import annotations

import torch

from . import _lib, ops
from ._lib import MM_I8

_FLOATS = (torch.float32, torch.bfloat16, torch.float16)


def _is_sdnq_tensor(weight) -> bool:
    return type(weight).__name__ == "SDNQTensor" or hasattr(weight, "sdnq_dequantizer")


def _check(input: torch.Tensor, weight: torch.Tensor, bias) -> None:
    if _is_sdnq_tensor(weight):
        raise NotImplementedError("SDNQTensor weights (quantized storage with its SVD and Hadamard branches) are not built for the int8 "
                                  "training matmul; pass a float weight")
    for name, t in (("input", input), ("weight", weight), ("bias", bias)):
        if t is not None and not t.is_cuda:
            raise _lib.SdnqHipError(f"the int8 training matmul needs {name} on a gfx950 device (got a CPU tensor); there is no CPU path")
    # each operand is quantized from its own dtype (the reference upcasts all of them to float32), so they need not agree: float32
    # master weights under 16-bit activations give y and grad_input in the input's dtype and grad_weight in grad_output's
    if input.dtype not in _FLOATS or weight.dtype not in _FLOATS or (bias is not None and bias.dtype not in _FLOATS):
        raise NotImplementedError(f"the int8 training matmul needs input, weight and bias each of float32 / bfloat16 / float16 "
                                  f"(got {input.dtype}, {weight.dtype}, {None if bias is None else bias.dtype})")
    if weight.ndim != 2 or input.shape[-1] != weight.shape[1]:
        raise ValueError(f"weight must be [out_features, in_features] matching input[..., in_features] (got {tuple(weight.shape)}, {tuple(input.shape)})")
    n, k = weight.shape
    if n % 16 or k % 16:
        raise NotImplementedError(f"the int8 training matmul is built for N % 16 == 0 and K % 16 == 0 (got N = {n}, K = {k})")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """`t` flattened to 2-D with 16-byte aligned rows of contiguous elements (what the quantizer kernels load)."""
    t = t.reshape(-1, t.shape[-1])
    if t.stride(1) != 1 or (t.stride(0) * t.element_size()) % 16 or t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _forward(x2d: torch.Tensor, weight: torch.Tensor, bias) -> torch.Tensor:
    xq, xs, _, _ = ops.rowquant(x2d, MM_I8)
    wq, ws, _, _ = ops.rowquant(_rows(weight), MM_I8)  # quantize_int_mm(weight.t(), dim=0): one scale per output row
    return ops.scaled_mm(MM_I8, xq, wq, xs, ws, bias, x2d.dtype)


def _backward(grad2d: torch.Tensor, xq_t, x_scale, wq_t, w_scale, need):
    """(grad_input [M,K], grad_weight [N,K], grad_bias [N]) from dY [M,N] and the column-quantized operands; None where `need` says so.
    A bias gradient without a weight gradient still runs the column pass over dY (for its colsum): rare, and the same bits either way."""
    dt = grad2d.dtype
    grad_input = grad_weight = grad_bias = None
    if need[0]:
        gq, gs, _, _ = ops.rowquant(grad2d, MM_I8)
        grad_input = ops.scaled_mm(MM_I8, gq, wq_t, gs, w_scale, None, dt)
    if need[1] or need[2]:
        gq_t, gs_t, colsum = ops.colquant_t(grad2d, want_colsum=bool(need[2]))
        if need[1]:
            grad_weight = ops.scaled_mm(MM_I8, gq_t, xq_t, gs_t, x_scale, None, dt)
        if need[2]:
            grad_bias = colsum.to(dt)
    return grad_input, grad_weight, grad_bias


class INT8MatmulDynamicBackward(torch.autograd.Function):
    """INT8MatmulDynamicBackward (linear_int8_dynamic.py:157-206): saves the float input and weight a requested gradient needs and
    quantizes them per column in the backward."""

    @staticmethod
    def forward(ctx, input, weight, bias=None):
        _check(input, weight, bias)
        x2d = _rows(input)
        out = _forward(x2d, weight, bias)
        ctx.input_shape = input.shape
        ctx.save_for_backward(x2d if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        return out.view(*input.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, grad_output):
        x2d, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        xq_t = x_scale = wq_t = w_scale = None
        if need[0]:
            wq_t, w_scale, _ = ops.colquant_t(_rows(weight))
        if need[1]:
            xq_t, x_scale, _ = ops.colquant_t(x2d)
        gi, gw, gb = _backward(_rows(grad_output), xq_t, x_scale, wq_t, w_scale, need)
        return (gi.view(ctx.input_shape) if gi is not None else None), gw, gb


class INT8MatmulDynamicBackwardCKPT(torch.autograd.Function):
    """INT8MatmulDynamicBackwardCKPT (linear_int8_dynamic_ckpt.py:76-132): W and x are quantized per column inside the forward and only
    their transposed int8 codes and float32 scales are saved -- one byte per element instead of two or four."""

    @staticmethod
    def forward(ctx, input, weight, bias=None):
        _check(input, weight, bias)
        x2d = _rows(input)
        out = _forward(x2d, weight, bias)
        xq_t = x_scale = wq_t = w_scale = None
        if ctx.needs_input_grad[0]:
            wq_t, w_scale, _ = ops.colquant_t(_rows(weight))
        if ctx.needs_input_grad[1]:
            xq_t, x_scale, _ = ops.colquant_t(x2d)
        ctx.input_shape = input.shape
        ctx.save_for_backward(xq_t, wq_t, x_scale, w_scale)
        return out.view(*input.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, grad_output):
        xq_t, wq_t, x_scale, w_scale = ctx.saved_tensors
        gi, gw, gb = _backward(_rows(grad_output), xq_t, x_scale, wq_t, w_scale, ctx.needs_input_grad)
        return (gi.view(ctx.input_shape) if gi is not None else None), gw, gb


int8_matmul_dynamic_with_backward = INT8MatmulDynamicBackward.apply
int8_matmul_dynamic_with_backward_ckpt = INT8MatmulDynamicBackwardCKPT.apply


def int8_matmul_dynamic(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, svd_up=None, svd_down=None,
                        hadamard=None, output_shape=None, do_input_reshape: bool = True, rotate_weight: bool = False,
                        use_sr: bool = False) -> torch.Tensor:
    """int8_matmul_dynamic (linear_int8_dynamic.py:85-115) for a float weight [N][K]: the forward product alone, no autograd graph."""
    if svd_up is not None or svd_down is not None:
        raise NotImplementedError("SVD factors in the int8 training matmul are not built")
    if hadamard is not None or rotate_weight:
        raise NotImplementedError("the Hadamard rotation in the int8 training matmul is not built")
    if use_sr:
        raise NotImplementedError("use_sr (stochastic rounding) is not built")
    if not do_input_reshape:
        raise NotImplementedError("do_input_reshape=False (the reference's own backward calls) is served by "
                                  "int8_matmul_dynamic_with_backward, not as a separate entry point")
    _check(input, weight, bias)
    with torch.no_grad():
        out = _forward(_rows(input), weight, bias)
    return out.view(output_shape if output_shape is not None else (*input.shape[:-1], weight.shape[0]))


def _few_rows(input: torch.Tensor) -> bool:
    return torch.numel(input) / input.shape[-1] < 32


def quantized_linear_forward_int8_matmul_dynamic(self, input: torch.Tensor) -> torch.Tensor:
    """linear_int8_dynamic.py:209-215."""
    if _few_rows(input):
        if _is_sdnq_tensor(self.weight):
            raise NotImplementedError("SDNQTensor weights are not built for the training Linear (quantized_linear_with_backward)")
        return torch.nn.functional.linear(input, self.weight, self.bias)
    return int8_matmul_dynamic_with_backward(input, self.weight, self.bias)


def quantized_linear_forward_int8_matmul_dynamic_ckpt(self, input: torch.Tensor) -> torch.Tensor:
    """linear_int8_dynamic_ckpt.py:135-141."""
    if _few_rows(input):
        if _is_sdnq_tensor(self.weight):
            raise NotImplementedError("SDNQTensor weights are not built for the training Linear (quantized_linear_with_backward)")
        return torch.nn.functional.linear(input, self.weight, self.bias)
    return int8_matmul_dynamic_with_backward_ckpt(input, self.weight, self.bias)


def _not_built(name: str, what: str):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"{name}: {what} is not built (the dynamic int8 training matmul is: int8_matmul_dynamic_with_backward)")
    fn.__name__ = fn.__qualname__ = name
    return fn


# the other training matmuls of the reference's package, importable from its module paths (sdnq/training/layers/linear/linear_*/*.py
# are views of these names): a caller that reaches one learns what is missing instead of computing in float
NOT_BUILT = {
    "int8_matmul_with_backward": "the static int8 training matmul (linear_int8.py, SDNQTensor weights)",
    "int8_matmul_with_backward_ckpt": "the static int8 training matmul (linear_int8_ckpt.py, SDNQTensor weights)",
    "fp8_matmul_with_backward": "the fp8 training matmul (linear_fp8.py)",
    "fp8_matmul_with_backward_ckpt": "the fp8 training matmul (linear_fp8_ckpt.py)",
    "fp8_matmul_dynamic_with_backward": "the dynamic fp8 training matmul (linear_fp8_dynamic.py)",
    "fp8_matmul_dynamic_with_backward_ckpt": "the dynamic fp8 training matmul (linear_fp8_dynamic_ckpt.py)",
    "uint8_matmul_with_backward": "the uint8 training matmul (linear_uint8.py)",
    "uint8_matmul_with_backward_ckpt": "the uint8 training matmul (linear_uint8_ckpt.py)",
    "uint8_matmul_dynamic_with_backward": "the dynamic uint8 training matmul (linear_uint8_dynamic.py)",
    "uint8_matmul_dynamic_with_backward_ckpt": "the dynamic uint8 training matmul (linear_uint8_dynamic_ckpt.py)",
    "fp16_matmul_with_backward": "the fp16 training matmul (linear_fp16.py)",
    "fp16_matmul_with_backward_ckpt": "the fp16 training matmul (linear_fp16_ckpt.py)",
    "fp16_matmul_dynamic_with_backward": "the dynamic fp16 training matmul (linear_fp16_dynamic.py)",
    "fp16_matmul_dynamic_with_backward_ckpt": "the dynamic fp16 training matmul (linear_fp16_dynamic_ckpt.py)",
}
globals().update({name: _not_built(name, what) for name, what in NOT_BUILT.items()})
