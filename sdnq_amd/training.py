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

The second half of the module is the other way of training on this package: adapters on a FROZEN quantized model --
``enable_input_grad(model)`` / ``QuantizedLinearInputGrad``, the input gradient through an accelerated quantized Linear layer, and with
``convs=True`` ``QuantizedConvInputGrad``, the same through quantized Conv1d / Conv2d layers.
"""
from __future__ import annotations

import torch

from . import _lib, linear, ops, scratch
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


# ---- input gradients through FROZEN quantized Linear layers (adapters on a quantized model) ---------------------------------------------
# The reference's QuantizedLinearBackward (training/layers/linear/forward.py): the forward is the layer, grad_input = grad_output @
# weight.dequantize().  Here the forward is the layer's own accelerated forward_func -- whatever it is: w8a8, fp8, uint8, float16 matmul,
# dequantize mode, the few-row branch, plans, linked projections -- so its output bits are the inference call's, and the backward decodes
# the stored codes transposed into the "operand" slot of sdnq_amd.scratch (ops.weight_t) and runs the float GEMM on it.  No float copy per
# layer: peak extra memory is one float copy of the LARGEST layer seen (two, the "decoded" slot, with SVD factors or a Hadamard rotation).
def _scratch(dev: torch.device, dtype: torch.dtype, numel: int, two: bool):
    """(operand, decoded | None) as 1-D tensors of `dtype` with at least `numel` elements: the "operand" and "decoded" slots of
    sdnq_amd.scratch.  "decoded" exists once a layer with SVD factors or a Hadamard rotation was seen and then has the size of "operand"."""
    have = scratch.held(dev)
    want = max(have["operand"].numel() if "operand" in have else 0, numel * dtype.itemsize)
    both = two or "decoded" in have
    bufs = scratch.take(dev, "input-gradient scratch", want, "operand", *(("decoded",) if both else ()))
    return bufs[0].view(dtype), (bufs[1].view(dtype) if both else None)


def _scratch_unfolded(dev: torch.device, dtype: torch.dtype, numel: int) -> torch.Tensor:
    """The whole "unfolded" slot as `dtype`, at least `numel` elements: the unfolded grad_output (one slab of U) of a conv backward."""
    return scratch.take(dev, "input-gradient scratch", numel * dtype.itemsize, "unfolded")[0].view(dtype)


def scratch_bytes(device=None) -> int:
    """Bytes the input-gradient and adapter scratch holds on `device` (default: the current one)."""
    return sum(b.numel() for b in scratch.held(torch.device("cuda" if device is None else device)).values())


def release_scratch() -> None:
    scratch.release()


def _weight_t_operand(layer, qw, dtype: torch.dtype, dev: torch.device) -> torch.Tensor:
    """ops.weight_t of a frozen layer -- W^T [K][N], SVD product added, Hadamard rotation undone -- in the "operand" slot."""
    dq = layer.sdnq_dequantizer
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    return ops.weight_t(qw, dtype, had, _scratch(dev, dtype, qw.n * qw.k, bool(qw.desc.svd_up) or had != 0))


def _linear_base_grad(layer, g2d: torch.Tensor) -> torch.Tensor:
    """grad_input [M][K] = dY . W of a frozen Linear layer, as QuantizedLinearInputGrad and the adapter of sdnq_amd.lora both compute it."""
    return ops.linear_float(g2d, _weight_t_operand(layer, linear._state(layer).qw, g2d.dtype, g2d.device), None)


def _check_grad_output(layer, grad_output: torch.Tensor, kind: str) -> None:
    """What every backward through a frozen quantized layer -- the input-gradient Functions here, the adapters of sdnq_amd.lora -- asks of
    grad_output: the layer's compute dtype (the backward products run in it), on the device.  kind: "Linear" or "conv", for the message."""
    dt = layer.sdnq_dequantizer.result_dtype
    if grad_output.dtype != dt:
        raise NotImplementedError(f"grad_output of dtype {grad_output.dtype} through a quantized {kind} whose compute dtype is {dt}: the "
                                  "backward products run in the layer's dtype")
    if not grad_output.is_cuda:
        raise _lib.SdnqHipError(f"gradients through a quantized {kind} need grad_output on a gfx950 device (got a CPU tensor)")


class QuantizedLinearInputGrad(torch.autograd.Function):
    """y = layer(input) with a graph: grad_input = dY . W, where W is the weight the layer's forward multiplies by (SVD product added,
    Hadamard rotation undone).  grad_bias = dY.sum(0) when the bias requires grad; the weight, scale, zero point and SVD factors are
    frozen and get none.  Saves the module and the input shape, no tensor.  Not differentiable twice."""

    @staticmethod
    def forward(ctx, layer, input, bias=None):
        if not input.is_cuda:
            raise _lib.SdnqHipError("input gradients through a quantized Linear need the input on a gfx950 device (got a CPU tensor); "
                                    "there is no CPU path")
        ctx.layer, ctx.input_shape = layer, input.shape
        ctx.bias_dtype = None if bias is None else bias.dtype
        with torch.no_grad():  # (autograd has switched gradients off here already: the layer takes the very path of an inference call)
            return layer.forward_func(layer, input)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        layer = ctx.layer
        _check_grad_output(layer, grad_output, "Linear")
        g2d = _rows(grad_output)
        grad_input = grad_bias = None
        if ctx.needs_input_grad[1]:
            if g2d.shape[0] == 0:
                grad_input = grad_output.new_zeros(ctx.input_shape)
            else:
                grad_input = _linear_base_grad(layer, g2d).view(ctx.input_shape)
        if ctx.needs_input_grad[2]:
            grad_bias = g2d.sum(0).to(ctx.bias_dtype)
        return None, grad_input, grad_bias


def quantized_linear_input_grad(layer, input: torch.Tensor) -> torch.Tensor:
    """`layer(input)` -- the output bits of the inference call -- with grad_input (and grad_bias) flowing back through the frozen layer."""
    from .linear import _attr
    return QuantizedLinearInputGrad.apply(layer, input, _attr(layer, "bias"))


# ---- the same through FROZEN quantized Conv1d / Conv2d layers ------------------------------------------------------------------------
# grad_x[b][ci][ih][iw] = sum over (co, i, j) of dY[b][co][oh][ow] * W[co][ci][i][j] with ih + p - i d = oh s (likewise w) runs as a gather
# and the float GEMM of the Linear backward:
#   U [B H W][kprod C_out]   ops.im2col_bwd (csrc/conv.hip): dY per INPUT pixel, columns (kernel position, channel), 0 where no tap exists
#   W^T                      ops.weight_t, [C_in kprod][C_out] with k = ci kprod + kpos -- viewed as [C_in][kprod C_out] it is the GEMM's
#                            [N][K] operand as it stands, contiguous along the reduction: no new weight kernel
#   grad2d [B H W][C_in]     = linear_float(U, W^T view); a torch permute takes it to NCHW as the forward's _folder does
# U is walked in slabs of rows so that its buffer stays bounded; every element of grad_x is rounded once, to the layer dtype.  Where the
# measurements say so (_takes_col2im_route: strided layers, few input positions) an ungrouped layer takes the kernels of the transposed
# convolution instead: cols = dY (NHWC) . W in float32 on the same weight operand, then ops.col2im.
CONV_GRAD_SLAB_MB = 256  # upper bound of the unfolded grad_output per launch pair; SDNQ_HIP_CONV_GRAD_SLAB_MB (read per call) overrides it.
# The default keeps every SDXL conv at batch 1 in one slab (the largest: 320 channels at 128 x 128, 16384 x 2880 bf16 = 94 MB).
_CONV_CLASSES = ("Conv1d", "Conv2d", "SDNQConv1d", "SDNQConv2d")


CONV_GRAD_ROUTE = None  # None: the rule of _takes_col2im_route; "gather" / "col2im" force one route (the tests and the benchmark tool do)


def _slab_rows(rows: int, row_bytes: int) -> int:
    """How many of `rows` units of `row_bytes` each a slab holds: at least one."""
    import os
    mb = float(os.environ.get("SDNQ_HIP_CONV_GRAD_SLAB_MB", "") or CONV_GRAD_SLAB_MB)
    return max(1, min(rows, int(mb * 2 ** 20) // row_bytes))


def _takes_col2im_route(groups: int, kprod: int, stride, rows: int) -> bool:
    """Which of the two routes to grad_x an ungrouped layer takes; a static rule of the geometry, from the measurements of
    tools/conv_input_grad_bench.py on an MI355X (profiles/conv_input_grad_bench.jsonl, bf16, batch 1, medians of graph replays, int8 /
    uint4 weights; `gather_route_us` against `col2im_route_us`):

      gather   im2col_bwd + float GEMM [B H W][C_in] over K = kprod C_out (this module's own route)
      col2im   the kernels of the transposed convolution: float32-out GEMM [B L_out][C_in kprod] over K = C_out, then ops.col2im

    * prod(stride) > 1, any kernel: the unfolded matrix of the gather route is 1 - 1 / prod(stride) zeros, which the GEMM multiplies all
      the same.  The SDXL down-samplers: 320 channels at 128 x 128, gather 108.9 / 113.3 us against col2im 88.2 / 90.6; 640 at 64 x 64,
      94.7 / 102.8 against 56.8 / 65.4.
    * B H W <= 1024 with a kernel larger than 1 x 1: the gather GEMM has 16 row tiles at most and C_in columns -- 80 to 320 tiles of a K loop
      kprod C_out long on 256 CUs -- where the col2im GEMM has C_in kprod columns.  1280 -> 1280 at 32 x 32: 94.1 / 122.2 against 87.9 / 116.4;
      640 -> 1280: 85.3 / 99.9 against 60.6 / 75.8; 2560 -> 1280: 156.1 / 212.7 against 153.6 / 210.7 (a tie inside the 2.5-3 % spread).
    Everywhere else the gather route won: 4096 input positions and more without a stride, 0.86x (320 -> 640 at 64 x 64: 68.2 against 79.3 us)
    to 0.39x (960 -> 320 at 128 x 128: 185.4 against 478.9) of the col2im route's time, whose float32 matrix is twice the bytes per element
    and kprod C_in wide; and 1 x 1 layers without a stride, where col2im is one more pass over the same GEMM (29.9 against 36.6).  The 1024
    is the one size measured on the col2im side of the line, the next size measured (4096) lies on the other: where between them the
    routes cross has not been measured.
    Grouped layers always gather: the col2im composition is built for groups == 1."""
    if groups != 1:
        return False
    if CONV_GRAD_ROUTE is not None:
        return CONV_GRAD_ROUTE == "col2im"
    return stride[0] * stride[1] > 1 or (kprod > 1 and rows <= 1024)


def _conv_geometry(layer):
    """(kernel, stride, padding, dilation, nd) of a Conv1d / Conv2d layer as the 2-D problem of conv._geometry (Conv1d: H = 1, kh = 1)."""
    from .conv import _pair
    dq = layer.sdnq_dequantizer
    nd = len(dq.original_shape) - 2
    if nd not in (1, 2) or isinstance(layer.padding, str) or layer.padding_mode != "zeros":
        raise NotImplementedError(input_grad_unsupported_reason(layer, convs=True) or "input gradients through this conv layer are not built")
    kernel = tuple(int(k) for k in dq.original_shape[2:])
    stride, padding, dilation = _pair(layer.stride, nd), _pair(layer.padding, nd), _pair(layer.dilation, nd)
    if nd == 1:
        kernel, stride, padding, dilation = (1, kernel[0]), (1, stride[0]), (0, padding[0]), (1, dilation[0])
    return kernel, stride, padding, dilation, nd


def _group_weights(layer, qw, groups: int):
    """The stored tensors of a plain grouped conv weight cut into one QuantWeight per conv group (rows g N_g .. (g + 1) N_g of the codes,
    scales and zero points; views, no copy unless a slab's codes do not start on 16 bytes), cached on the layer for as long as its kernel
    state lives.  None when the stored layout cannot be cut by rows: the caller then dequantizes the whole weight and transposes slabs."""
    cached = layer.__dict__.get("_sdnq_conv_grad_slabs")
    if cached is not None and cached[0] is qw:
        return cached[1]
    slabs = None
    codes, sc, zp = qw.keep[0], qw.keep[1], qw.keep[2]
    ng = qw.n // groups
    nbytes = codes.numel() * codes.element_size()
    # (every storage format keeps element e at bit e * bits of the stream, unpack_dev.h: a row slab is a byte range when the stream has no padding)
    if (codes.is_contiguous() and nbytes * 8 == qw.n * qw.k * int(qw.desc.bits) and sc.numel() % qw.n == 0
            and (zp is None or zp.numel() == sc.numel())):
        flat = codes.view(-1).view(torch.uint8)
        per_row, per_row_s = nbytes // qw.n, sc.numel() // qw.n
        slabs = []
        for g in range(groups):
            w_g = flat[g * ng * per_row:(g + 1) * ng * per_row]
            if w_g.data_ptr() % 16:
                w_g = w_g.clone()
            s_g = sc[g * ng * per_row_s:(g + 1) * ng * per_row_s]
            z_g = None if zp is None else zp[g * ng * per_row_s:(g + 1) * ng * per_row_s]
            d = _lib.SdnqWeight.from_buffer_copy(bytes(qw.desc))
            d.weight, d.scale, d.zero_point, d.n = w_g.data_ptr(), s_g.data_ptr(), (None if z_g is None else z_g.data_ptr()), ng
            slabs.append(ops.QuantWeight(desc=d, n=ng, k=qw.k, group_size=qw.group_size, keep=(w_g, s_g, z_g, None, None),
                                         scale_dtype=qw.scale_dtype))
    layer.__dict__["_sdnq_conv_grad_slabs"] = (qw, slabs)
    return slabs


def _conv_weight_operands(layer, qw, groups: int, dtype: torch.dtype, dev: torch.device):
    """[one per conv group] the weight operand [C_in / groups][kprod * C_out / groups] of the backward GEMM, all inside the "operand" slot
    of the scratch (the groups one after the other: together N * K elements, the size of the whole weight)."""
    dq = layer.sdnq_dequantizer
    ng, k = qw.n // groups, qw.k
    cg = int(dq.original_shape[1])
    if groups == 1:
        return [_weight_t_operand(layer, qw, dtype, dev).view(cg, (k // cg) * ng)]
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    slabs = None if qw.desc.svd_up or had else _group_weights(layer, qw, groups)
    first, second = _scratch(dev, dtype, qw.n * k, slabs is None)
    if slabs is None:
        # a Hadamard rotation (or a stored layout that cannot be cut by rows): the whole weight by the kernels of the forward, then one
        # transpose per group's row slab
        wd = ops.dequant(qw, dtype, had, out=second[:qw.n * k].view(qw.n, k))
        return [ops.transpose2d(wd[g * ng:(g + 1) * ng], out=first[g * ng * k:(g + 1) * ng * k]).view(cg, (k // cg) * ng) for g in range(groups)]
    return [ops.dequant_t(slabs[g], dtype, out=first[g * ng * k:(g + 1) * ng * k]).view(cg, (k // cg) * ng) for g in range(groups)]


def _conv_grad_input(layer, dy4: torch.Tensor, in_hw, kernel, stride, padding, dilation) -> torch.Tensor:
    """grad2d [B * H * W][C_in] (NHWC rows) of a conv layer from dY [B][C_out][H_out][W_out]: per slab of rows one im2col_bwd and one float
    GEMM per conv group into the slab's rows of grad2d."""
    dq = layer.sdnq_dequantizer
    groups = int(layer.groups)
    dt, dev = dy4.dtype, dy4.device
    b, cout = dy4.shape[0], dy4.shape[1]
    cg, kprod = int(dq.original_shape[1]), kernel[0] * kernel[1]
    ng, kc = cout // groups, kprod * cout
    rows = b * in_hw[0] * in_hw[1]
    slab = _slab_rows(rows, kc * dt.itemsize)
    operands = _conv_weight_operands(layer, linear._state(layer).qw, groups, dt, dev)
    ubuf = _scratch_unfolded(dev, dt, slab * kc)
    grad2d = torch.empty((rows, cg * groups), device=dev, dtype=dt)
    for r0 in range(0, rows, slab):
        n = min(slab, rows - r0)
        u = ops.im2col_bwd(dy4, in_hw, kernel, stride, padding, dilation, row0=r0, rows=n, out=ubuf, groups=groups)
        for g, wt in enumerate(operands):
            ops.linear_float_into(u[:, g * kprod * ng:(g + 1) * kprod * ng], wt, None, grad2d[r0:r0 + n], g * cg)
    return grad2d


def _conv_grad_input_col2im(layer, dy4: torch.Tensor, in_shape, kernel, stride, padding, dilation, dy2d=None) -> torch.Tensor:
    """grad_x [B][C_in][H][W] of an ungrouped conv layer by the kernels of the transposed convolution: cols[(b, oh, ow)][(ci, kpos)] =
    dY (NHWC) . W in float32 -- the weight operand is ops.weight_t's [C_in kprod][C_out] as it stands -- then every input pixel gathers the
    taps that reach it (ops.col2im): float32 sums, one rounding.  `cols` lives in the "unfolded" scratch slot, whole images per slab (one
    image at least, whatever the bound says).  dy2d: the NHWC copy of dY [B L_out][C_out] where the caller has made it already."""
    qw = linear._state(layer).qw
    dt, dev = dy4.dtype, dy4.device
    b, cout, ho, wo = dy4.shape
    cin, h, w = in_shape[1], in_shape[2], in_shape[3]
    wt = _weight_t_operand(layer, qw, dt, dev)
    per_image = ho * wo * qw.k
    imgs = _slab_rows(b, per_image * 4)
    cols = _scratch_unfolded(dev, torch.float32, imgs * per_image)
    if dy2d is None:
        dy2d = dy4.permute(0, 2, 3, 1).contiguous().view(b * ho * wo, cout)
    pieces = []
    for b0 in range(0, b, imgs):
        n = min(imgs, b - b0)
        c = cols[:n * per_image].view(n * ho * wo, qw.k)
        ops.linear_float_f32_into(dy2d[b0 * ho * wo:(b0 + n) * ho * wo], wt, c, 0)
        pieces.append(ops.col2im(c, None, dt, n, cin, (ho, wo), (h, w), kernel, stride, padding, dilation))
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=0)


def _conv_base_grad(layer, dy4: torch.Tensor, shape4, kernel, stride, padding, dilation, dy2d=None):
    """grad_x of a frozen conv layer on the route _takes_col2im_route picks, as QuantizedConvInputGrad and the conv adapter of
    sdnq_amd.lora both compute it: ("col2im", grad_x [B][C_in][H][W]) or ("gather", grad2d [B H W][C_in] -- NHWC rows, which the caller
    permutes to NCHW).  dy4 [B][C_out][H_out][W_out], shape4 = (B, C_in, H, W); dy2d: see _conv_grad_input_col2im."""
    in_hw = (shape4[2], shape4[3])
    if _takes_col2im_route(int(layer.groups), kernel[0] * kernel[1], stride, shape4[0] * in_hw[0] * in_hw[1]):
        return "col2im", _conv_grad_input_col2im(layer, dy4, shape4, kernel, stride, padding, dilation, dy2d)
    return "gather", _conv_grad_input(layer, dy4, in_hw, kernel, stride, padding, dilation)


class QuantizedConvInputGrad(torch.autograd.Function):
    """y = layer(input) with a graph, for a frozen quantized Conv1d / Conv2d layer with zero padding: grad_input is the backward-data
    convolution of dY with W, the weight the layer's forward multiplies by (SVD product added, Hadamard rotation undone), computed as
    ops.im2col_bwd + the float GEMM on ops.weight_t's operand; grad_bias = dY.sum over batch and space when the bias requires grad; the
    weight, scale, zero point and SVD factors are frozen and get none.  Saves the module and the input shape, no tensor.  Not differentiable
    twice."""

    @staticmethod
    def forward(ctx, layer, input, bias=None):
        if not input.is_cuda:
            raise _lib.SdnqHipError("input gradients through a quantized conv need the input on a gfx950 device (got a CPU tensor); "
                                    "there is no CPU path")
        ctx.layer, ctx.input_shape = layer, input.shape
        ctx.bias_dtype = None if bias is None else bias.dtype
        with torch.no_grad():  # (autograd has switched gradients off here already: the layer takes the very path of an inference call)
            return layer.forward_func(layer, input)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        layer = ctx.layer
        _check_grad_output(layer, grad_output, "conv")
        kernel, stride, padding, dilation, nd = _conv_geometry(layer)
        shape = tuple(ctx.input_shape)
        if len(shape) != nd + 2:
            raise NotImplementedError(f"input gradients through a quantized conv need a batched input [B, C, *spatial] (got shape {shape})")
        grad_input = grad_bias = None
        if ctx.needs_input_grad[1]:
            if grad_output.numel() == 0 or 0 in shape:
                grad_input = grad_output.new_zeros(shape)
            else:
                dy4 = grad_output.unsqueeze(2) if nd == 1 else grad_output
                in_hw = (1, shape[2]) if nd == 1 else (shape[2], shape[3])
                route, grad_input = _conv_base_grad(layer, dy4, (shape[0], shape[1], *in_hw), kernel, stride, padding, dilation)
                if route == "gather":
                    grad_input = grad_input.view(shape[0], *in_hw, shape[1]).permute(0, 3, 1, 2).contiguous()
                grad_input = grad_input.view(shape)  # (Conv1d: the H = 1 axis goes)
        if ctx.needs_input_grad[2]:
            grad_bias = grad_output.sum(dim=[0] + list(range(2, grad_output.ndim))).to(ctx.bias_dtype)
        return None, grad_input, grad_bias


def quantized_conv_input_grad(layer, input: torch.Tensor) -> torch.Tensor:
    """`layer(input)` -- the output bits of the inference call -- with grad_input (and grad_bias) flowing back through the frozen conv."""
    from .linear import _attr
    return QuantizedConvInputGrad.apply(layer, input, _attr(layer, "bias"))


def _conv_input_grad_reason(module, dq, cls) -> str | None:
    from .support import unsupported_reason
    if isinstance(getattr(module, "padding", 0), str) or getattr(module, "padding_mode", "zeros") != "zeros":
        return (f"{cls}: input gradients are built for zero padding given as numbers (got padding={getattr(module, 'padding', None)!r}, "
                f"padding_mode={getattr(module, 'padding_mode', None)!r})")
    fwd = getattr(module, "forward_func", None)
    if getattr(fwd, "__module__", None) not in ("sdnq_amd.conv", __name__):
        return "the layer does not run on the MI355X forwards (call sdnq_amd.accelerate(model) first)"
    why = unsupported_reason(module)
    if why is not None:
        return why
    shape = tuple(int(d) for d in dq.original_shape)
    groups = int(getattr(module, "groups", 1))
    kprod = 1
    for d in shape[2:]:
        kprod *= d
    if groups < 1 or shape[0] % groups:
        return f"{cls}: groups = {groups} does not divide the {shape[0]} output channels"
    k, ng = shape[1] * kprod, shape[0] // groups
    # sdnq_hip_dequant_t / sdnq_hip_transpose2d decode 16-runs of a stored row (K = C_in / groups * prod(kernel)) and leave 16-byte runs along
    # the output channels of a group (8 values); with 8 | C_out / groups the GEMM's reduction C_out / groups * prod(kernel) is a multiple of
    # 8 as well, which is what sdnq_hip_linear_float asks of it (16-byte rows), and any width C_in / groups is served
    if k % 16 or ng % 8:
        return (f"input gradients need 16 | C_in / groups * prod(kernel) and 8 | C_out / groups (got {k}, {ng}; reduction "
                f"C_out / groups * prod(kernel) = {ng * kprod}, width C_in / groups = {shape[1]}): the transposed weight leaves in 16-byte runs")
    if kprod * shape[0] > 64 * 65535:
        return f"input gradients need prod(kernel) * C_out <= {64 * 65535} (got {kprod * shape[0]}): the launch grid of the unfold"
    if dq.result_dtype not in _FLOATS:
        return f"layer dtype {dq.result_dtype} is not built for input gradients (float32, bfloat16, float16 are)"
    return None


def input_grad_unsupported_reason(module, convs: bool = False) -> str | None:
    """None when `enable_input_grad` serves `module` (an SDNQ layer); otherwise the sentence that says why not.  convs: judge Conv1d /
    Conv2d layers as `enable_input_grad(model, convs=True)` does."""
    from .common import linear_types
    from .support import unsupported_reason
    dq = module.sdnq_dequantizer
    cls = getattr(dq, "layer_class_name", None)
    if cls not in linear_types:
        if not convs:
            return f"{cls}: input gradients are built for quantized Linear layers (conv, transposed-conv and embedding layers are not)"
        if cls not in _CONV_CLASSES:
            return (f"{cls}: input gradients are built for quantized Linear, Conv1d and Conv2d layers (Conv3d, transposed-conv and embedding "
                    "layers are not)")
        return _conv_input_grad_reason(module, dq, cls)
    why = unsupported_reason(module)
    if why is not None:
        return why
    fwd = getattr(module, "forward_func", None)
    if getattr(fwd, "__module__", None) not in ("sdnq_amd.linear", __name__):
        return "the layer does not run on the MI355X forwards (call sdnq_amd.accelerate(model) first)"
    n, k = dq.out_features, dq.in_features
    if k % 16 or n % 8:
        return f"input gradients need 16 | K and 8 | N (got K = {k}, N = {n}): the transposed weight leaves in 16-byte runs"
    if dq.result_dtype not in _FLOATS:
        return f"layer dtype {dq.result_dtype} is not built for input gradients (float32, bfloat16, float16 are)"
    return None


def _with_input_grad(fwd, route=quantized_linear_input_grad):
    grad_on = torch.is_grad_enabled

    def forward(self, input):
        if grad_on() and input.requires_grad:
            return route(self, input)  # (its forward comes back here with gradients off)
        return fwd(self, input)
    forward.__name__ = forward.__qualname__ = getattr(fwd, "__name__", "forward") + "_with_input_grad"
    forward._sdnq_inference_forward = fwd
    return forward


class InputGradResult(int):
    """What `enable_input_grad()` returns: an int (the number of layers switched) that also carries `.enabled` and `.skipped` --
    [(qualified module name, reason)] of the SDNQ layers that still cut the graph."""

    def __new__(cls, enabled: int, skipped):
        r = super().__new__(cls, enabled)
        r.enabled, r.skipped = int(enabled), list(skipped)
        return r

    def __iter__(self):  # `n, skipped = enable_input_grad(model)`
        return iter((self.enabled, self.skipped))


def enable_input_grad(model: torch.nn.Module, enabled: bool = True, convs: bool = False) -> InputGradResult:
    """Let gradients flow to what is upstream of the frozen quantized Linear layers of an accelerated `model` (adapters, LoRA).

    Wraps the ``forward_func`` of every accelerated quantized Linear: a call made with gradients enabled on an input that requires grad
    goes through ``QuantizedLinearInputGrad`` (same output bits, grad_input = dY . W on HIP kernels, no float weight kept); every other
    call takes the forward the layer had, plans included, for the price of one Python check.  Conv, transposed-conv and embedding layers,
    layers with K % 16 != 0 or N % 8 != 0 and layers outside float32 / bfloat16 / float16 are left alone and listed in ``.skipped`` and in
    ONE ``warnings.warn``: the graph is still cut there.  ``enabled=False`` puts the forwards back.  Re-pointing a layer's forward
    afterwards (``apply_sdnq_options_to_model``, ``accelerate``) drops the switch for that layer.  Out of scope: ``torch.compile`` of the
    wrapped forward and double backward.

    ``convs=True`` wraps the accelerated quantized Conv1d / Conv2d layers as well (``QuantizedConvInputGrad``: the backward-data convolution
    as ``ops.im2col_bwd`` + the same float GEMM, grouped layers one GEMM per group) -- what a UNet quantized with ``quant_conv=True`` needs,
    whose ResNet convs otherwise cut the graph between all its attention blocks.  Left alone and listed, each with its sentence: Conv3d,
    transposed convs, embeddings, string padding and padding modes other than zeros, layers whose C_in / groups * prod(kernel) is no
    multiple of 16 or whose C_out / groups is no multiple of 8.  Extra memory of a conv backward: the weight operand in the buffers of the
    Linear layers plus one slab of the unfolded grad_output, at most ``SDNQ_HIP_CONV_GRAD_SLAB_MB`` (default ``CONV_GRAD_SLAB_MB`` = 256)
    megabytes; all of it is counted by ``scratch_bytes()`` and freed by ``release_scratch()``.  Ungrouped layers with a stride, and ungrouped
    layers larger than 1 x 1 on at most 1024 input positions, take the kernels of the transposed convolution instead (float32-out GEMM +
    ``ops.col2im``, its float32 matrix in the same "unfolded" slot, whole images per slab): the rule and the measurements behind it are at
    ``_takes_col2im_route``; both routes round every element once.  The default stays ``convs=False``: nothing changes for callers that do
    not ask."""
    count, skipped = 0, []
    for name, module in model.named_modules():
        if getattr(module, "sdnq_dequantizer", None) is None:
            continue
        fwd = getattr(module, "forward_func", None)
        inner = getattr(fwd, "_sdnq_inference_forward", None)
        if not enabled:
            if inner is not None:
                module.forward_func = inner
                count += 1
            continue
        if inner is not None:  # switched already
            count += 1
            continue
        try:
            why = input_grad_unsupported_reason(module, convs=convs)
        except Exception as e:  # noqa: BLE001  a foreign record the predicate cannot read: leave the layer alone
            why = f"{type(e).__name__} while reading the layer's record: {e}"
        if why is not None:
            skipped.append((name or type(module).__name__, why))
            continue
        is_conv = getattr(module.sdnq_dequantizer, "layer_class_name", None) in _CONV_CLASSES
        module.forward_func = _with_input_grad(fwd, quantized_conv_input_grad if is_conv else quantized_linear_input_grad)
        count += 1
    if skipped:
        import warnings
        warnings.warn(f"sdnq_amd.enable_input_grad: {len(skipped)} SDNQ layer(s) still cut the autograd graph (nothing upstream of them "
                      "receives a gradient): " + "; ".join(f"{n} ({w})" for n, w in skipped[:8]) + (" ..." if len(skipped) > 8 else ""),
                      stacklevel=2)
    return InputGradResult(count, skipped)
