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
``enable_input_grad(model)`` / ``QuantizedLinearInputGrad``, the input gradient through an accelerated quantized Linear layer.
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


# ---- input gradients through FROZEN quantized Linear layers (adapters on a quantized model) ---------------------------------------------
# The reference's QuantizedLinearBackward (training/layers/linear/forward.py): the forward is the layer, grad_input = grad_output @
# weight.dequantize().  Here the forward is the layer's own accelerated forward_func -- whatever it is: w8a8, fp8, uint8, float16 matmul,
# dequantize mode, the few-row branch, plans, linked projections -- so its output bits are the inference call's, and the backward decodes
# the stored codes transposed into ONE scratch buffer per device (ops.weight_t) and runs the float GEMM on it.  No float copy per layer:
# peak extra memory is one float copy of the LARGEST layer seen (two when a layer has SVD factors or a Hadamard rotation).
_SCRATCH = {}  # device index -> [first, second | None]: uint8 buffers, grown to the largest layer seen and reused by every layer


def _scratch(dev: torch.device, dtype: torch.dtype, numel: int, two: bool):
    """(first, second | None) as 1-D tensors of `dtype` with at least `numel` elements.  `second` exists once a layer with SVD factors or a
    Hadamard rotation was seen and then has the size of `first`.  The buffers are used in stream order by the stream the backward runs on
    (autograd runs a node's backward on its forward's stream); a model whose backwards run on several streams at once is not served."""
    nbytes = numel * dtype.itemsize
    bufs = _SCRATCH.setdefault(dev.index if dev.index is not None else torch.cuda.current_device(), [None, None])
    have = 0 if bufs[0] is None else bufs[0].numel()
    want = max(have, nbytes)
    grow = [i for i in range(2) if (i == 0 or two or bufs[1] is not None) and (bufs[i] is None or bufs[i].numel() < want)]
    if grow and torch.cuda.is_current_stream_capturing():
        raise _lib.SdnqHipError("input-gradient scratch: run one eager backward before capturing a graph (the buffer is not sized yet)")
    for i in grow:
        bufs[i] = None  # (the old block goes back to the allocator before the new one is taken)
        bufs[i] = torch.empty(want, device=dev, dtype=torch.uint8)
    return bufs[0].view(dtype), (None if bufs[1] is None else bufs[1].view(dtype))


def scratch_bytes(device=None) -> int:
    """Bytes the input-gradient scratch holds on `device` (default: the current one)."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    return sum(b.numel() for b in _SCRATCH.get(idx, ()) if b is not None)


def release_scratch() -> None:
    _SCRATCH.clear()


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
        from . import linear
        layer = ctx.layer
        dq = layer.sdnq_dequantizer
        if grad_output.dtype != dq.result_dtype:
            raise NotImplementedError(f"grad_output of dtype {grad_output.dtype} through a quantized Linear whose compute dtype is "
                                      f"{dq.result_dtype}: the backward GEMM runs in the layer's dtype")
        if not grad_output.is_cuda:
            raise _lib.SdnqHipError("input gradients through a quantized Linear need grad_output on a gfx950 device (got a CPU tensor)")
        g2d = _rows(grad_output)
        grad_input = grad_bias = None
        if ctx.needs_input_grad[1]:
            if g2d.shape[0] == 0:
                grad_input = grad_output.new_zeros(ctx.input_shape)
            else:
                qw = linear._state(layer).qw
                had = dq.hadamard_group_size if dq.use_hadamard else 0
                scratch = _scratch(g2d.device, g2d.dtype, qw.n * qw.k, bool(qw.desc.svd_up) or had != 0)
                grad_input = ops.linear_float(g2d, ops.weight_t(qw, g2d.dtype, had, scratch), None).view(ctx.input_shape)
        if ctx.needs_input_grad[2]:
            grad_bias = g2d.sum(0).to(ctx.bias_dtype)
        return None, grad_input, grad_bias


def quantized_linear_input_grad(layer, input: torch.Tensor) -> torch.Tensor:
    """`layer(input)` -- the output bits of the inference call -- with grad_input (and grad_bias) flowing back through the frozen layer."""
    from .linear import _attr
    return QuantizedLinearInputGrad.apply(layer, input, _attr(layer, "bias"))


def input_grad_unsupported_reason(module) -> str | None:
    """None when `enable_input_grad` serves `module` (an SDNQ layer); otherwise the sentence that says why not."""
    from .common import linear_types
    from .support import unsupported_reason
    dq = module.sdnq_dequantizer
    cls = getattr(dq, "layer_class_name", None)
    if cls not in linear_types:
        return f"{cls}: input gradients are built for quantized Linear layers (conv, transposed-conv and embedding layers are not)"
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


def _with_input_grad(fwd):
    grad_on = torch.is_grad_enabled

    def forward(self, input):
        if grad_on() and input.requires_grad:
            return quantized_linear_input_grad(self, input)  # (its forward comes back here with gradients off)
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


def enable_input_grad(model: torch.nn.Module, enabled: bool = True) -> InputGradResult:
    """Let gradients flow to what is upstream of the frozen quantized Linear layers of an accelerated `model` (adapters, LoRA).

    Wraps the ``forward_func`` of every accelerated quantized Linear: a call made with gradients enabled on an input that requires grad
    goes through ``QuantizedLinearInputGrad`` (same output bits, grad_input = dY . W on HIP kernels, no float weight kept); every other
    call takes the forward the layer had, plans included, for the price of one Python check.  Conv, transposed-conv and embedding layers,
    layers with K % 16 != 0 or N % 8 != 0 and layers outside float32 / bfloat16 / float16 are left alone and listed in ``.skipped`` and in
    ONE ``warnings.warn``: the graph is still cut there.  ``enabled=False`` puts the forwards back.  Re-pointing a layer's forward
    afterwards (``apply_sdnq_options_to_model``, ``accelerate``) drops the switch for that layer.  Out of scope: ``torch.compile`` of the
    wrapped forward and double backward."""
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
            why = input_grad_unsupported_reason(module)
        except Exception as e:  # noqa: BLE001  a foreign record the predicate cannot read: leave the layer alone
            why = f"{type(e).__name__} while reading the layer's record: {e}"
        if why is not None:
            skipped.append((name or type(module).__name__, why))
            continue
        module.forward_func = _with_input_grad(fwd)
        count += 1
    if skipped:
        import warnings
        warnings.warn(f"sdnq_amd.enable_input_grad: {len(skipped)} SDNQ layer(s) still cut the autograd graph (nothing upstream of them "
                      "receives a gradient): " + "; ".join(f"{n} ({w})" for n, w in skipped[:8]) + (" ..." if len(skipped) > 8 else ""),
                      stacklevel=2)
    return InputGradResult(count, skipped)
