"""Trainable low-rank adapters (LoRA) on the frozen quantized Linear -- and Conv1d / Conv2d -- layers of an accelerated model, fused on HIP kernels.

    y = layer(x) + scale * (x . down^T) . up^T          down [rank][K], up [N][rank], scale = alpha / rank

``add_lora(model)`` registers ``lora_down`` / ``lora_up`` on every accelerated quantized Linear it serves and replaces the layer's
``forward_func`` by a wrapper of this module.  The wrapper's base is the layer's own inference forward -- w8a8, fp8, uint8, the float16
matmul, dequantize mode, the few-row branch, plans, linked projections -- so with ``up == 0`` the output bits are the inference call's.
Per call:

    forward      y   = base(layer, x)                          the layer's own route
                 t   = ops.lowrank_down(x, down)               [M][rank], rounded to the layer dtype
                 y  += scale * t . up^T                         ops.lowrank_add, in place, one rounding of y
    backward     g_t = ops.lowrank_down(dY, up^T)              [M][rank]; its matrix-core kernel needs 16 | N: a layer with N % 16 == 8 (which
                                                               add_lora serves) takes sdnq_hip_linear_float's few-row kernel there --
                                                               the same values, much slower; not measured
                 grad_input = ops.linear_float(dY, W^T)        training._linear_base_grad: ops.weight_t into the "operand" scratch slot
                 grad_input += scale * g_t . down              ops.lowrank_add, in place: one more rounding of grad_input
                 grad_up    = scale * dY^T . t                 ops.lowrank_grad, [N][rank]
                 grad_down  = scale * g_t^T . x                ops.lowrank_grad(out_t=True), [rank][K]
                 grad_bias  = dY.sum(0)                        when the bias requires grad

``add_lora(model, dropout=p)`` is PEFT's ``lora_dropout``: y = layer(x) + scale * B(A(dropout(x))), on the adapter branch only, in training
mode only (``module.training`` and p > 0, with or without gradients, as nn.Dropout).  No mask and no dropped copy of x is ever written: the
mask is a pure function of (seed, offset, element index) -- Philox4x32-10 in the counter convention of the AdamW step, stream 5
(include/sdnq_hip.h) -- and the three kernels that need it recompute it for the 16-byte chunk they move:

    forward      t   = ops.lowrank_down_dropout(x, down)       the mask on the fragments of x in registers
                 y  += scale_d * t . up^T                       ops.lowrank_add, unchanged
    backward     g_t = ops.lowrank_down(dY, up^T)              unchanged
                 grad_up    = scale_d * dY^T . t                ops.lowrank_grad, unchanged
                 grad_down  = scale_d * g_t^T . (mask * x)      ops.lowrank_grad_dropout: the mask on x as it is staged
                 grad_input = dY . W + scale_d * mask * (g_t . down)   ops.lowrank_add_dropout: the mask in the epilogue

An element is dropped iff its 16 random bits are below T = min(65535, max(1, round(p * 65536))) (``dropout_threshold``): the effective
probability is T / 65536, within 2^-17 of p (at least 2^-16).  The survivors are not rescaled in the operand; 1 / (1 - p) goes into the
float32 scale the kernels take anyway, scale_d = float32(scale * 65536 / (65536 - T)) (``dropout_scale``).  Each forward call reads
(initial_seed, offset) from torch's device generator and advances the offset by 4, as ``sdnq_amd.optim`` does for its stochastic stores;
the backward keeps (T, seed, offset) as three Python ints beside what it saves anyway.  ``torch.cuda.manual_seed`` reproduces a run, and
``torch.utils.checkpoint`` (which restores the generator state for its recomputation) replays the same mask.  While a stream is being
captured an active dropout raises (the offset is drawn on the host: a replay would repeat one mask); ``dropout=0`` and ``eval()`` capture
as before.  ``eval()`` and ``dropout=0`` run exactly the calls above without the mask: the same entry points and bits as before.

The wrapper handles input gradients itself; ``enable_input_grad`` called afterwards leaves these layers alone (it lists them as running
a forward that is not its own).  The parameters go to ``sdnq_amd.optim.AdamW`` (``add_lora(...).parameters``).

``add_lora(model, convs=True)`` serves the accelerated quantized Conv1d / Conv2d layers as well (groups == 1, zero padding), in PEFT's form:
lora_A a conv with the layer's kernel, stride, padding and dilation from C_in to rank channels (``lora_down`` [rank, C_in, *kernel]), lora_B
a 1 x 1 conv from rank to C_out (``lora_up`` [C_out, rank, 1(, 1)]).  With L = H_out W_out, M = B L and the free 2-D views of the factors:

    forward      y   = base(layer, x)                          the layer's own route, NCHW
                 t   = ops.conv_lowrank_down(x, down2d)        [M][rank] = im2col(x) . down2d^T without the unfolded matrix
                 y_b += scale * up2d . t_b^T                    per image, ops.lowrank_add with its operands swapped on y_b [C_out][L]; where 8
                                                               does not divide L: on an NHWC copy of y, copied back (two more passes of data
                                                               movement, the same single rounding)
    backward     dy2d = dY as NHWC rows [M][C_out]             made once, shared with the col2im route of the base gradient
                 g_t  = ops.lowrank_down(dy2d, up2d^T)         [M][rank]
                 grad_up    = scale * dy2d^T . t               ops.lowrank_grad
                 grad_down  = scale * g_t^T . im2col(x)        ops.conv_lowrank_grad, [rank][C_in kprod]
                 grad_input = QuantizedConvInputGrad's base gradient (training._conv_base_grad, either of its routes)
                              + scale * conv^T(g_t, down)      ops.im2col_bwd of g_t and ops.lowrank_add in place (one more rounding) where
                                                               kprod rank <= 256 and the rows are 16-byte pieces, ops.linear_float + add (two
                                                               more) elsewhere: _conv_adapter_grad_input
                 grad_bias  = dY.sum over batch and space

``add_lora(model, use_dora=True)`` is PEFT's ``use_dora`` (weight-decomposed LoRA) on the Linear adapters.  Each adapted layer gets a
trainable magnitude ``lora_magnitude`` m [N] (float32), and with W [N][K] the weight the layer's forward multiplies by (what ``ops.dequant``
returns: SVD product added, Hadamard rotation undone), s = lora_scale:

    normsq[n] = sum_k ( W[n][k] + s * sum_r up[n][r] down[r][k] )^2    ops.dora_normsq: float32, from the STORED CODES in one launch -- each
                                                                       e = fma(s, acc, w32), the rank sum on the matrix cores, no [N][K]
                                                                       tensor; DETACHED, as PEFT's weight_norm.  Always s, never the
                                                                       dropout scale or a mask (PEFT's lora_weight is B @ A).  A layer with
                                                                       SVD factors or a rotation: ops.dequant into the "decoded" scratch slot
                                                                       + ops.dora_normsq_dense (one more pass over the weight)
    c[n]      = m[n] / sqrt(normsq[n])                                 torch ops on [N]: autograd turns grad_c into grad_m
    y         = c * ( W x + s_d * up (down (mask * x)) ) + b           the layer's own route, ops.lowrank_down(_dropout), then
                                                                       ops.lowrank_add_dora in place: with z the base output and acc = t . up^T,
                                                                       y = round(fma(c s_d, acc, fma(c - 1, z - b, z))), c s_d and c - 1 one
                                                                       float32 operation each
    backward  g = round(dY * c), q[n] = sum_i dY[i][n] (y[i][n] - b[n])   ops.dora_bwd: one pass over dY and the SAVED OUTPUT y (y - b = c * u;
                                                                       slabs of 256 rows in a fixed order, no atomics)
              grad_c = q / c where c != 0, else 0                      a magnitude entry that is exactly zero gets gradient 0
              g_t, grad_input, grad_up, grad_down                      the chain above with g in place of dY (dropout variants included)
              grad_bias = dY.sum(0)                                    the unscaled dY

m is initialised to sqrt(normsq) by the same kernel (up == 0: || W[n,:] ||), so c == 1.0f exactly and a layer that has never taken an
optimizer step returns the bits of the inference call.  normsq is recomputed on every call and never cached: ``sdnq_amd.optim`` writes the
parameters through raw pointers without bumping ``_version``.  The wrapper runs the same three kernels under ``torch.no_grad()`` / ``eval()``.
Measured (tools/dora_bench.py, profiles/dora_bench.jsonl): see README.md.

``merge_lora(model)`` folds the adapters into the STORED CODES of their layers (PEFT's ``merge_and_unload``) and takes them off, and
``merge_lora_state_dict(model, sd, scale)`` applies a PEFT-keyed LoRA file to a quantized model that carries no adapters -- what UIs do on
every LoRA switch.  Both go through ``_merge_layer``: ``ops.merge_lowrank`` reads the codes once and writes the re-quantized codes, scales
and zero points of c * (W + s * up @ down) in one launch (csrc/merge.hip: e in registers as the norm kernel forms it, then the quantizer's
arithmetic; nothing of size N x K in float exists), bit for bit what ``ops.quantize_weight`` gives on the float32 matrix e.  SVD layers keep
their factors (the codes are the residual); Hadamard layers merge ``ops.hadamard(down)`` (the codes are those of the rotated weight; one
more rounding of down to the layer dtype); what the kernel is not built for -- group sizes other than 16 .. 256 and row-wise, codebooks,
ranks above 256 -- takes ``ops.dequant`` + ``torch.addmm`` + ``ops.quantize_weight`` / ``quantize_codebook``.  LOSSY (the codes are
re-quantized: up to half a step of the new scales) and there is no unmerge; a per-layer error report, merging conv adapters and merging
DoRA onto layers with SVD factors are not built (listed in ``.skipped``, adapters left on).

Not built, each raising or listed with its sentence: adapters on grouped and 3-D convs, on transposed-conv and embedding layers and on float32
layers, on convs with string padding or a padding mode other than zeros; dropout on conv adapters; DoRA on conv adapters, caching the norm of
frozen adapters; per-layer ranks, rsLoRA; ``torch.compile`` of the wrapper (a compiled model runs it inside the opaque whole-layer operator: the values of adapter
inference, no gradients) and double backward; the C++ fast plans calling the adapter (the wrapper calls the base forward, which keeps its
plan); a batched (single-launch) NCHW add of the conv adapter's up projection (one ops.lowrank_add launch per image).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib, linear, ops, scratch, training
from .linear import _attr

_DTYPES = (torch.bfloat16, torch.float16)


def _workspace(dev: torch.device, nbytes: int):
    """The float32 partial sums of ops.lowrank_grad / ops.conv_lowrank_grad: the "partials" slot of sdnq_amd.scratch, None for no bytes."""
    return scratch.take(dev, "adapter scratch", nbytes, "partials")[0] if nbytes else None


def _factor_grad(a: torch.Tensor, b: torch.Tensor, scale: float, out_t: bool, out_dtype: torch.dtype, drop=None) -> torch.Tensor:
    """scale * a^T . b; drop: None or the triple of _draw_dropout -- a under its dropout mask."""
    ws = _workspace(a.device, ops.lowrank_grad_workspace_bytes(a.shape[0], a.shape[1], b.shape[1])) if a.shape[0] else None
    if drop is None:
        return ops.lowrank_grad(a, b, scale, out_t=out_t, out_dtype=out_dtype, workspace=ws)
    return ops.lowrank_grad_dropout(a, b, scale, *drop, out_t=out_t, out_dtype=out_dtype, workspace=ws)


def _check_call(layer, input: torch.Tensor) -> torch.dtype:
    dt = layer.sdnq_dequantizer.result_dtype
    if not input.is_cuda:
        raise _lib.SdnqHipError("a quantized Linear with an adapter needs its input on a gfx950 device (got a CPU tensor); there is no CPU path")
    if input.dtype != dt:
        raise NotImplementedError(f"input of dtype {input.dtype} through an adapter on a layer whose compute dtype is {dt}: the adapter "
                                  "products run in the layer's dtype")
    return dt


def dropout_threshold(p: float) -> int:
    """T of ``add_lora(dropout=p)``: an element is dropped iff its 16 random bits are < T = min(65535, max(1, round(p * 65536))) -- the
    effective probability is T / 65536."""
    return min(65535, max(1, round(float(p) * 65536)))


def dropout_scale(scale: float, threshold: int) -> float:
    """scale_d = float32(scale * 65536 / (65536 - T)), the quotient in double: the adapter's scale with the 1 / (1 - p) of the survivors."""
    return ctypes.c_float(float(scale) * 65536.0 / (65536 - int(threshold))).value


def _draw_dropout(layer, dev: torch.device):
    """None when dropout is off for this call; otherwise ops._Dropout(T, seed, offset), the triple in the order every entry point takes it
    -- (initial_seed, offset) of torch's device generator, whose offset advances by 4 (torch keeps it a multiple of 4), as
    SDNQOptimizer.step draws for its stochastic stores."""
    p = float(getattr(layer, "lora_dropout", 0.0))
    if p <= 0.0 or not layer.training:
        return None
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("adapter dropout draws its (seed, offset) on the host and cannot be captured in a graph: a replay would repeat "
                           "one mask; capture with model.eval() or add_lora(dropout=0)")
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, offset = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(offset + 4)
    return ops._Dropout(dropout_threshold(p), seed, offset)


def _scale(layer, drop) -> float:
    return layer.lora_scale if drop is None else dropout_scale(layer.lora_scale, drop.threshold)


def _run(layer, base, input: torch.Tensor, down: torch.Tensor, up: torch.Tensor, drop=None, dora=None):
    """(y, x2d, t): the three steps of the forward with gradients off.  down / up: the factors in the layer dtype.  drop: None or the
    triple of _draw_dropout -- then t comes from the masked x and the scale carries 1 / (1 - p).  dora: None or (c [N] float32,
    bias in the layer dtype | None) -- then the add is ops.lowrank_add_dora."""
    y = base(layer, input)
    x2d = training._rows(input)
    n = up.shape[0]
    if x2d.shape[0] == 0:
        return y, x2d, x2d.new_empty((0, down.shape[0]))
    t = ops.lowrank_down(x2d, down) if drop is None else ops.lowrank_down_dropout(x2d, down, *drop)
    try:
        y2d = y.view(-1, n)
    except RuntimeError:
        y = y.contiguous()
        y2d = y.view(-1, n)
    # in place unless the rows cannot be moved in 16-byte pieces or several of them are one piece of memory (an expanded view)
    ld = ops._ld(y2d)  # (a single row: its length, whatever stride torch reports for the size-1 axis)
    if y2d.stride(1) != 1 or ld < n or y2d.data_ptr() % 16 or (ld * y2d.element_size()) % 16:
        y = y.clone(memory_format=torch.contiguous_format)
        y2d = y.view(-1, n)
    if dora is None:
        ops.lowrank_add(t, up, y2d, _scale(layer, drop))
    else:
        ops.lowrank_add_dora(t, up, y2d, _scale(layer, drop), *dora)
    return y, x2d, t


def _zero_grads(grad_output: torch.Tensor, input_shape, need_x: bool, *params):
    """The gradients of a call without rows: (zeros of `input_shape` in grad_output's dtype, or None without `need_x`; then for each of
    `params` -- a factor or c where its gradient is needed, None where not -- zeros like it, or None)."""
    return (grad_output.new_zeros(input_shape) if need_x else None, *(None if p is None else torch.zeros_like(p) for p in params))


def _project_grad(g2d: torch.Tensor, up2d: torch.Tensor) -> torch.Tensor:
    """g_t [M][rank] = g2d . up2d, up2d [N][rank] cast to the dtype of g2d: ops.lowrank_down on its transpose."""
    return ops.lowrank_down(g2d, up2d.to(g2d.dtype).t().contiguous())


def _linear_forward(ctx, layer, base, input, down, up, bias, c=None):
    """The forward of QuantizedLinearLoRA (c None) and of QuantizedLinearDoRA (c [N] float32).  Saves x2d, t, down, up -- and with c: c,
    the OUTPUT y and the bias (None without one).  Without c nothing of DoRA is touched: plain LoRA's entry points and saved tensors."""
    dt = _check_call(layer, input)
    ctx.drop = drop = _draw_dropout(layer, input.device)
    with torch.no_grad():
        if c is not None:
            c = c.detach().contiguous()
        y, x2d, t = _run(layer, base, input, down.detach().to(dt), up.detach().to(dt), drop, None if c is None else (c, _dora_bias(bias, dt)))
    ctx.layer, ctx.input_shape = layer, input.shape
    ctx.bias_dtype = None if bias is None else bias.dtype
    ctx.save_for_backward(x2d, t, down, up, *(() if c is None else (c, y, bias)))
    return y


def _linear_backward(ctx, grad_output, need_x, need_down, need_up, need_c, need_bias):
    """(grad_input, grad_down, grad_up, grad_c, grad_bias), None where not needed: the backward chain of the module docstring, once for
    both Linear Functions.  A forward that saved c (DoRA) first turns dY into g = round(dY * c) (ops.dora_bwd, with q for grad_c only
    where the magnitude needs a gradient) and runs the chain on g; grad_bias comes from the unscaled dY either way."""
    layer = ctx.layer
    x2d, t, down, up, *dora = ctx.saved_tensors
    training._check_grad_output(layer, grad_output, "Linear")
    dy2d = training._rows(grad_output)
    drop = ctx.drop
    dt, scale = dy2d.dtype, _scale(layer, drop)
    grad_c = grad_bias = None
    m, n = dy2d.shape
    if m == 0:
        grad_input, grad_down, grad_up, grad_c = _zero_grads(grad_output, ctx.input_shape, need_x, down if need_down else None,
                                                              up if need_up else None, dora[0] if need_c else None)
    else:
        grad_input = grad_down = grad_up = None
        g2d = dy2d
        if dora:
            c, y, bias = dora
            ws = _workspace(dy2d.device, ops.dora_bwd_workspace_bytes(m, n)) if need_c else None
            g2d, q = ops.dora_bwd(dy2d, training._rows(y) if need_c else None, _dora_bias(bias, dt), c, want_q=need_c, workspace=ws)
            if need_c:
                grad_c = torch.where(c != 0, q / c, torch.zeros_like(q))
        g_t = None
        if need_x or need_down:
            g_t = _project_grad(g2d, up)
        if need_x:
            gi2d = training._linear_base_grad(layer, g2d)
            if drop is None:
                ops.lowrank_add(g_t, down.to(dt).t().contiguous(), gi2d, scale)
            else:
                ops.lowrank_add_dropout(g_t, down.to(dt).t().contiguous(), gi2d, scale, *drop)
            grad_input = gi2d.view(ctx.input_shape)
        if need_up:
            grad_up = _factor_grad(g2d, t, scale, False, up.dtype)
        if need_down:
            grad_down = _factor_grad(x2d, g_t, scale, True, down.dtype, drop)
    if need_bias:
        grad_bias = dy2d.sum(0).to(ctx.bias_dtype)
    return grad_input, grad_down, grad_up, grad_c, grad_bias


class QuantizedLinearLoRA(torch.autograd.Function):
    """y = layer(input) + scale * (input . down^T) . up^T with a graph: gradients for the input, the two factors and the bias; the
    weight, scale, zero point and SVD factors of the layer are frozen and get none.  Saves the module, the flattened input and t -- and,
    with dropout active, the three ints (T, seed, offset) from which the backward's kernels recompute the mask.  Not differentiable
    twice."""

    @staticmethod
    def forward(ctx, layer, base, input, down, up, bias=None):
        return _linear_forward(ctx, layer, base, input, down, up, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        _, _, need_x, need_down, need_up, need_bias = ctx.needs_input_grad
        grad_input, grad_down, grad_up, _, grad_bias = _linear_backward(ctx, grad_output, need_x, need_down, need_up, False, need_bias)
        return None, None, grad_input, grad_down, grad_up, grad_bias


# ---- DoRA (add_lora(..., use_dora=True)) ------------------------------------------------------------------------------------------------
def _layer_normsq(layer, down, up, scale=None) -> torch.Tensor:
    """normsq [N] float32 of a Linear layer: sum_k (W[n][k] + lora_scale * (up . down)[n][k])^2 -- down / up in the layer dtype, or both None
    for || W[n,:] ||^2.  A plain layer: ops.dora_normsq on the stored codes.  A layer with SVD factors or a Hadamard rotation: ops.dequant
    into the "decoded" slot of sdnq_amd.scratch and ops.dora_normsq_dense on it (one more pass over the weight).  scale: instead of the
    layer's lora_scale (merge_lora_state_dict: a layer without an adapter)."""
    qw = linear._state(layer).qw
    dq = layer.sdnq_dequantizer
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    scale = (layer.lora_scale if scale is None else scale) if up is not None else 1.0  # (without factors the scale multiplies nothing)
    if not qw.desc.svd_up and not had:
        return ops.dora_normsq(qw, up, down, scale)
    dt = dq.result_dtype
    nk = qw.n * qw.k
    _, decoded = training._scratch(qw.keep[0].device, dt, nk, True)
    return ops.dora_normsq_dense(ops.dequant(qw, dt, had, out=decoded[:nk].view(qw.n, qw.k)), up, down, scale)


def _dora_bias(bias, dt: torch.dtype):
    """The bias as the DoRA kernels read it: the layer dtype, contiguous, 16-byte aligned (None stays None)."""
    if bias is None:
        return None
    b = bias.detach().to(dt).contiguous()
    return b.clone() if b.data_ptr() % 16 else b


def _dora_c(layer, down: torch.Tensor, up: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """c [N] float32 = lora_magnitude / sqrt(normsq), normsq recomputed by the norm kernel on every call and detached (PEFT's
    weight_norm.detach()): plain torch ops on [N], so autograd turns grad_c into the gradient of the magnitude."""
    with torch.no_grad():
        normsq = _layer_normsq(layer, down.detach().to(dt), up.detach().to(dt))
    return _attr(layer, "lora_magnitude") / torch.sqrt(normsq)


class QuantizedLinearDoRA(torch.autograd.Function):
    """y = c . (W x + scale * up . (down . x)) + b with a graph, c [N] float32 an INPUT (the wrapper computes it from lora_magnitude and the
    detached norm): gradients for the input, the two factors, c and the bias.  Saves x2d, t, down, up, c, the OUTPUT y and the bias; the
    backward recovers c . u = y - b from the saved output (the op that consumes y usually saves the same tensor), so
        g      = round(dY * c),  q[n] = sum_i dY[i][n] (y[i][n] - b[n])        ops.dora_bwd, one pass
        grad_c = q / c where c != 0, else 0                                    (a magnitude entry that is exactly zero gets gradient 0)
        g_t, grad_input, grad_up, grad_down: the chain QuantizedLinearLoRA runs, on g (_linear_backward; dropout variants included)
        grad_bias = dY.sum(0)                                                  the unscaled dY
    Not differentiable twice."""

    @staticmethod
    def forward(ctx, layer, base, input, down, up, c, bias=None):
        return _linear_forward(ctx, layer, base, input, down, up, bias, c)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        return (None, None, *_linear_backward(ctx, grad_output, *ctx.needs_input_grad[2:]))


# ---- the same on frozen quantized Conv1d / Conv2d layers (add_lora(..., convs=True)) ----------------------------------------------------
# PEFT's conv adapter: lora_A is a conv with the layer's kernel, stride, padding and dilation from C_in to rank channels, lora_B a 1 x 1
# conv from rank to C_out.  On the unfolded activation U = im2col(x) [M = B L][K = C_in kprod] (L = H_out W_out) it is the Linear adapter:
# t = U . down2d^T, y += scale * t . up2d^T -- but the layer's forward never writes U in float (its w8a8 route writes int8 codes), and U
# is kprod times the bytes of x.  ops.conv_lowrank_down / ops.conv_lowrank_grad (csrc/conv_lowrank.hip) read x itself; on the eleven SDXL
# conv problems of tools/conv_lora_bench.py (bf16, batch 1, ranks 16 and 64; profiles/conv_lora_bench.jsonl) they take 0.28 - 0.92 and
# 0.33 - 0.87 of the time of ops.im2col + the Linear adapter's kernel, so no layer takes that composition.
def _conv_check_call(layer, input: torch.Tensor, nd: int) -> torch.dtype:
    dt = layer.sdnq_dequantizer.result_dtype
    if not input.is_cuda:
        raise _lib.SdnqHipError("a quantized conv with an adapter needs its input on a gfx950 device (got a CPU tensor); there is no CPU path")
    if input.dtype != dt:
        raise NotImplementedError(f"input of dtype {input.dtype} through an adapter on a conv whose compute dtype is {dt}: the adapter "
                                  "products run in the layer's dtype")
    if input.ndim != nd + 2:
        raise NotImplementedError(f"a quantized conv with an adapter needs a batched input [B, C, *spatial] (got shape {tuple(input.shape)})")
    return dt


def _conv_run(layer, base, input: torch.Tensor, down: torch.Tensor, up: torch.Tensor, geometry):
    """(y, x4, t): the three steps of the conv forward with gradients off.  down [rank, C_in, *kernel] / up [C_out, rank, 1(, 1)]: the
    factors in the layer dtype.  y comes from the layer's own route in NCHW; with 8 | L the up projection is added there, per image, by
    ops.lowrank_add with its operands swapped -- y_b [C_out][L] += scale * up2d . t_b^T: one read, one write and one rounding of y.
    Otherwise (the rows of y_b are not 16-byte pieces) y is copied to NHWC rows, ops.lowrank_add runs in its usual orientation and the
    result is copied back: two more passes of pure data movement, the same single rounding.  Either way an exactly zero sum keeps the
    element's bits (up == 0: the inference call's output)."""
    kernel, stride, padding, dilation, nd = geometry
    y = base(layer, input)
    x4 = input.unsqueeze(2) if nd == 1 else input
    rank, n = down.shape[0], up.shape[0]
    if y.numel() == 0:
        return y, x4, y.new_empty((0, rank))
    t = ops.conv_lowrank_down(x4, down.reshape(rank, -1), kernel, stride, padding, dilation)[0]
    up2d = up.reshape(n, rank)
    b = y.shape[0]
    l = y.numel() // (b * n)
    if not y.is_contiguous():
        y = y.contiguous()
    if l % 8 == 0 and y.data_ptr() % 16 == 0:
        y3 = y.view(b, n, l)
        for i in range(b):
            ops.lowrank_add(up2d, t[i * l:(i + 1) * l], y3[i], layer.lora_scale)
        return y, x4, t
    rows = y.view(b, n, l).permute(0, 2, 1).contiguous().view(b * l, n)
    ops.lowrank_add(t, up2d, rows, layer.lora_scale)
    return rows.view(b, l, n).permute(0, 2, 1).contiguous().view(y.shape), x4, t


def _conv_adapter_grad_input(route: str, gi: torch.Tensor, g_t: torch.Tensor, down: torch.Tensor, shape4, out_shape, geometry, scale: float):
    """grad_x [B][C_in][H][W] = (the base gradient `gi` of training._conv_base_grad's `route`) + scale * conv^T(g_t, down), the adapter
    term from existing kernels: g_t as [B][rank][H_out][W_out] goes through ops.im2col_bwd -- U_g [B H W][kprod rank], columns (kernel
    position, r), in the "unfolded" scratch slot, which the base gradient is done with -- and meets down rearranged to [C_in][kprod rank].
    Roundings of an element, after the base gradient's own one:
      kprod rank <= 256, gather route, 8 | C_in     ops.lowrank_add on the NHWC rows, before the permute: ONE more
      kprod rank <= 256, col2im route, 8 | H W      ops.lowrank_add per image with its operands swapped, on the NCHW result: ONE more
      elsewhere                                     ops.linear_float rounds the term to the layer dtype, torch's add_ rounds the sum: TWO more"""
    kernel, stride, padding, dilation, _ = geometry
    b, cin, h, w = shape4
    _, ho, wo = out_shape
    rank, kprod = down.shape[0], kernel[0] * kernel[1]
    kr = kprod * rank
    g4 = g_t.view(b, ho, wo, rank).permute(0, 3, 1, 2).contiguous()
    u = ops.im2col_bwd(g4, (h, w), kernel, stride, padding, dilation,
                       out=training._scratch_unfolded(g_t.device, g_t.dtype, b * h * w * kr))
    d = down.reshape(rank, cin, kprod).permute(1, 2, 0).reshape(cin, kr).contiguous()
    if route == "gather":  # gi: NHWC rows [B H W][C_in]
        if kr <= 256 and cin % 8 == 0:
            ops.lowrank_add(u, d, gi, scale)
        else:
            gi.add_(ops.linear_float(u, d, None), alpha=scale)
        return gi.view(b, h, w, cin).permute(0, 3, 1, 2).contiguous()
    hw = h * w
    if kr <= 256 and hw % 8 == 0 and gi.is_contiguous() and gi.data_ptr() % 16 == 0:
        g3 = gi.view(b, cin, hw)
        for i in range(b):
            ops.lowrank_add(d, u[i * hw:(i + 1) * hw], g3[i], scale)
        return gi
    return gi.add_(ops.linear_float(u, d, None).view(b, h, w, cin).permute(0, 3, 1, 2), alpha=scale)


class QuantizedConvLoRA(torch.autograd.Function):
    """y = layer(input) + scale * B(A(input)) with a graph, for a frozen quantized Conv1d / Conv2d layer (groups == 1, zero padding):
    gradients for the input, the two factors and the bias; the weight, scale, zero point and SVD factors of the layer are frozen and get
    none.  Saves the module, the input (as [B, C, H, W]) and t.  Backward, with dy2d the NHWC copy of dY (made once, shared with the
    col2im route of the base gradient):
        g_t        = ops.lowrank_down(dy2d, up2d^T)                          [M][rank]
        grad_up    = scale * dy2d^T . t                                      ops.lowrank_grad
        grad_down  = scale * g_t^T . im2col(x)                               ops.conv_lowrank_grad
        grad_input = training._conv_base_grad (QuantizedConvInputGrad's, either route) + scale * conv^T(g_t, down)  (_conv_adapter_grad_input)
        grad_bias  = dY.sum over batch and space
    Not differentiable twice."""

    @staticmethod
    def forward(ctx, layer, base, input, down, up, bias=None):
        geometry = training._conv_geometry(layer)
        dt = _conv_check_call(layer, input, geometry[4])
        with torch.no_grad():
            y, x4, t = _conv_run(layer, base, input, down.detach().to(dt), up.detach().to(dt), geometry)
        ctx.layer, ctx.input_shape, ctx.geometry = layer, input.shape, geometry
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.save_for_backward(x4, t, down, up)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        layer = ctx.layer
        x4, t, down, up = ctx.saved_tensors
        training._check_grad_output(layer, grad_output, "conv")
        kernel, stride, padding, dilation, nd = ctx.geometry
        dt, scale = grad_output.dtype, layer.lora_scale
        _, _, need_x, need_down, need_up, need_bias = ctx.needs_input_grad
        grad_bias = None
        if grad_output.numel() == 0 or 0 in ctx.input_shape:
            grad_input, grad_down, grad_up = _zero_grads(grad_output, ctx.input_shape, need_x, down if need_down else None,
                                                         up if need_up else None)
        else:
            grad_input = grad_down = grad_up = None
            dy4 = (grad_output.unsqueeze(2) if nd == 1 else grad_output).contiguous()
            b, n, ho, wo = dy4.shape
            rank = down.shape[0]
            dy2d = dy4.permute(0, 2, 3, 1).contiguous().view(b * ho * wo, n)
            g_t = None
            if need_x or need_down:
                g_t = _project_grad(dy2d, up.reshape(n, rank))
            if need_x:
                shape4 = tuple(x4.shape)
                route, gi = training._conv_base_grad(layer, dy4, shape4, kernel, stride, padding, dilation, dy2d)
                grad_input = _conv_adapter_grad_input(route, gi, g_t, down.to(dt), shape4, (b, ho, wo), ctx.geometry, scale).view(ctx.input_shape)
            if need_up:
                grad_up = _factor_grad(dy2d, t, scale, False, up.dtype).view(up.shape)
            if need_down:
                ws = _workspace(x4.device, ops.conv_lowrank_grad_workspace_bytes(x4.shape, kernel, stride, padding, dilation, rank))
                grad_down = ops.conv_lowrank_grad(x4, g_t, kernel, stride, padding, dilation, scale, out_dtype=down.dtype, workspace=ws).view(down.shape)
        if need_bias:
            grad_bias = grad_output.sum(dim=[0] + list(range(2, grad_output.ndim))).to(ctx.bias_dtype)
        return None, None, grad_input, grad_down, grad_up, grad_bias


# ---- the forwards add_lora installs ------------------------------------------------------------------------------------------------------
def _wrapper(suffix: str, with_graph, without_graph, names=("lora_down", "lora_up")):
    """wrap(base, previous) -> the forward_func of a layer with an adapter.  Per call: `with_graph(layer, base, input, *parameters)` -- an
    autograd Function -- when gradients are on and the input or one of the layer's parameters `names` requires one, else
    `without_graph(...)` under torch.no_grad(): the same kernels without a Function.  The forward is stamped with the name of `base` plus
    `suffix` and with what remove_lora and add_lora read: _sdnq_lora_base, the inference forward it calls, and _sdnq_lora_previous, the
    forward_func it replaced."""
    def wrap(base, previous):
        grad_on = torch.is_grad_enabled

        def forward(self, input):
            params = [_attr(self, name) for name in names]
            if grad_on() and (input.requires_grad or any(p.requires_grad for p in params)):
                return with_graph(self, base, input, *params)
            with torch.no_grad():
                return without_graph(self, base, input, *params)
        forward.__name__ = forward.__qualname__ = getattr(base, "__name__", "forward") + suffix
        forward._sdnq_lora_base, forward._sdnq_lora_previous = base, previous
        return forward
    return wrap


def _lora_graph(layer, base, input, down, up):
    return QuantizedLinearLoRA.apply(layer, base, input, down, up, _attr(layer, "bias"))


def _lora_plain(layer, base, input, down, up):
    dt = _check_call(layer, input)
    return _run(layer, base, input, down.detach().to(dt), up.detach().to(dt), _draw_dropout(layer, input.device))[0]


def _dora_graph(layer, base, input, down, up, magnitude):
    dt = _check_call(layer, input)
    return QuantizedLinearDoRA.apply(layer, base, input, down, up, _dora_c(layer, down, up, dt), _attr(layer, "bias"))


def _dora_plain(layer, base, input, down, up, magnitude):
    dt = _check_call(layer, input)
    c = _dora_c(layer, down, up, dt).contiguous()
    return _run(layer, base, input, down.detach().to(dt), up.detach().to(dt), _draw_dropout(layer, input.device),
                (c, _dora_bias(_attr(layer, "bias"), dt)))[0]


def _conv_graph(layer, base, input, down, up):
    return QuantizedConvLoRA.apply(layer, base, input, down, up, _attr(layer, "bias"))


def _conv_plain(layer, base, input, down, up):
    geometry = training._conv_geometry(layer)
    dt = _conv_check_call(layer, input, geometry[4])
    return _conv_run(layer, base, input, down.detach().to(dt), up.detach().to(dt), geometry)[0]


_with_lora = _wrapper("_with_lora", _lora_graph, _lora_plain)
_with_dora = _wrapper("_with_dora", _dora_graph, _dora_plain, ("lora_down", "lora_up", "lora_magnitude"))
_with_conv_lora = _wrapper("_with_lora", _conv_graph, _conv_plain)


def _refresh_compile_plan(module) -> None:
    """Under torch.compile SDNQLayer.forward traces a planned layer as rowquant + matmul operators, which never reach forward_func;
    torch_ops.layer_plan gives a layer that carries an adapter no such plan (whoever derives it: here, accelerate, a deepcopy), so it
    traces as the ONE opaque whole-layer operator, which calls the wrapper: the values of adapter inference, no gradients there."""
    if "_sdnq_hip_plan" in module.__dict__:
        from . import torch_ops
        try:
            module.__dict__["_sdnq_hip_plan"] = torch_ops.layer_plan(module)
        except Exception:  # noqa: BLE001  (as torch_ops.layer_handle: the whole-layer operator handles a module the rule cannot read)
            module.__dict__["_sdnq_hip_plan"] = None


def lora_unsupported_reason(module, convs: bool = False) -> str | None:
    """None when `add_lora` serves `module` (an SDNQ layer); otherwise the sentence that says why not.  convs: judge Conv1d / Conv2d
    layers as `add_lora(model, convs=True)` does."""
    from .common import linear_types
    cls = getattr(module.sdnq_dequantizer, "layer_class_name", None)
    conv = cls not in linear_types
    if conv and not convs:
        return f"{cls}: adapters are built for quantized Linear layers (conv, transposed-conv and embedding layers are not)"
    if conv and cls not in training._CONV_CLASSES:
        return (f"{cls}: adapters are built for quantized Linear, Conv1d and Conv2d layers (Conv3d, transposed-conv and embedding "
                "layers are not)")
    if getattr(getattr(module, "forward_func", None), "_sdnq_lora_base", None) is not None:
        return "the layer carries an adapter already (remove_lora(model) takes it off)"
    if conv and int(getattr(module, "groups", 1)) != 1:
        return f"{cls} with groups = {int(module.groups)}: conv adapters are built for groups == 1 (grouped convs are not)"
    why = training.input_grad_unsupported_reason(module, convs=conv)
    if why is not None:
        return why
    dt = module.sdnq_dequantizer.result_dtype
    if dt not in _DTYPES:
        return f"layer dtype {dt}: adapters are built for bfloat16 and float16 layers (float32 layers are not)"
    return None


class LoRAResult(int):
    """What `add_lora()` returns: an int (the number of layers that got an adapter) that also carries `.added`, `.skipped` --
    [(qualified module name, reason)] of the SDNQ layers left without one -- and `.parameters`, the new nn.Parameters in module order
    (down, up per layer): the list to hand to ``sdnq_amd.optim.AdamW``."""

    def __new__(cls, added: int, skipped, parameters):
        r = super().__new__(cls, added)
        r.added, r.skipped, r.parameters = int(added), list(skipped), list(parameters)
        return r


def _selected(targets):
    if targets is None:
        return lambda name: True
    if callable(targets):
        return targets
    subs = [targets] if isinstance(targets, str) else list(targets)
    return lambda name: any(s in name for s in subs)


def add_lora(model: torch.nn.Module, rank: int = 16, alpha: float | None = None, targets=None, dtype: torch.dtype | None = None,
             seed: int | None = None, convs: bool = False, dropout: float = 0.0, use_dora: bool = False) -> LoRAResult:
    """Put a trainable rank-`rank` adapter on every accelerated quantized Linear of `model` whose qualified name `targets` selects
    (None: all; a list of substrings; or a predicate on the name).

    Registers ``module.lora_down`` [rank, K] (kaiming-uniform as nn.Linear initialises its weight, drawn from `seed` in module order)
    and ``module.lora_up`` [N, rank] (zeros) as nn.Parameters of `dtype` (default: the layer's dtype; torch.float32 for master weights,
    cast to the layer dtype per call), stores ``module.lora_scale = (alpha or rank) / rank`` and replaces ``forward_func`` (see the module
    docstring; a layer switched by ``enable_input_grad`` before is unwrapped to its inference forward -- the adapter's own backward
    computes the input gradient).  Served: what ``training.input_grad_unsupported_reason`` accepts (16 | K, 8 | N, running on the MI355X
    forwards) in bfloat16 or float16.  float32 layers, conv and embedding layers are left alone and listed in ``.skipped`` and in ONE
    ``warnings.warn``.  8 <= rank <= 256, rank % 8 == 0.  Re-pointing a layer's forward afterwards (``accelerate``,
    ``apply_sdnq_options_to_model``) takes the adapter off that layer's forward, eager and compiled alike, as it drops the switch of
    ``enable_input_grad``: the parameters stay registered until ``remove_lora``; call ``add_lora`` after those, not before.

    ``convs=True`` serves the accelerated quantized Conv1d / Conv2d layers as well (``QuantizedConvLoRA``): those that
    ``training.input_grad_unsupported_reason(module, convs=True)`` accepts, with ``groups == 1``, in bfloat16 or float16.  Their parameters
    have PEFT's shapes: ``lora_down`` [rank, C_in, *kernel] (lora_A, a conv with the layer's geometry; kaiming-uniform with bound
    1 / sqrt(C_in * prod(kernel)), from `seed` in module order with the Linear layers) and ``lora_up`` [C_out, rank, 1(, 1)] (lora_B, a
    1 x 1 conv; zeros).  Grouped convs, Conv3d, transposed convs, embeddings, float32 layers, string padding and padding modes other than
    zeros are listed in ``.skipped``, each with its sentence.  The default leaves every conv layer alone, as before.

    ``dropout`` (0 <= dropout < 1, PEFT's ``lora_dropout``; stored as ``module.lora_dropout``) drops elements of the adapter branch's
    input in training mode, fused into the adapter kernels (module docstring): the effective probability is
    ``dropout_threshold(dropout) / 65536``; each call draws (seed, offset) from torch's device generator, so ``torch.cuda.manual_seed``
    reproduces a run and ``torch.utils.checkpoint``, which restores the generator state, recomputes with the same mask.  0.0, the
    default, changes nothing.  With ``convs=True`` a dropout > 0 raises NotImplementedError before any module is touched.

    ``use_dora=True`` is PEFT's ``use_dora`` (weight-decomposed LoRA; module docstring): every adapted Linear also gets
    ``module.lora_magnitude`` [N] -- ALWAYS float32, whatever `dtype` says (a 16-bit magnitude would lose c == 1 at initialisation) --
    initialised to || W[n,:] || by the norm kernel itself, appended to ``.parameters`` after the layer's lora_down and lora_up, and
    ``module.lora_dora = True``.  The norm is recomputed by the kernel on EVERY call, never cached: ``sdnq_amd.optim`` updates parameters
    through raw pointers without bumping ``_version``, so a cache keyed on the factors would go stale silently (caching for frozen adapters
    is not built).  A layer with an all-zero weight row (norm 0) is listed in ``.skipped`` and gets no adapter.  A magnitude entry that is
    exactly zero makes u unrecoverable from the saved output: its gradient is reported as 0.  With ``convs=True`` it raises
    NotImplementedError before any module is touched.  False, the default, runs exactly the code and entry points of plain LoRA."""
    dropout = float(dropout)
    if not 0.0 <= dropout < 1.0:
        raise ValueError(f"add_lora: 0 <= dropout < 1 (got dropout = {dropout})")
    if convs and dropout > 0.0:
        raise NotImplementedError("add_lora: dropout on conv adapters is not built (the conv adapter kernels have no mask); call "
                                  "add_lora(..., convs=True) with dropout=0, or add_lora(..., dropout=p) for the Linear layers alone")
    if convs and use_dora:
        raise NotImplementedError("add_lora: DoRA on conv adapters is not built (the norm kernel reads Linear weights, the conv add has no "
                                  "column-scale epilogue); call add_lora(..., convs=True) with use_dora=False, or add_lora(..., "
                                  "use_dora=True) for the Linear layers alone")
    if rank % 8 or not 8 <= rank <= 256:
        raise ValueError(f"add_lora: rank % 8 == 0 and 8 <= rank <= 256 (got rank = {rank}): the adapter kernels move 16-byte rank chunks")
    if dtype is not None and dtype not in (torch.float32, *_DTYPES):
        raise ValueError(f"add_lora: dtype must be None (the layer's), torch.float32, torch.bfloat16 or torch.float16 (got {dtype})")
    from .common import linear_types
    pick = _selected(targets)
    gen = None if seed is None else torch.Generator().manual_seed(int(seed))
    scale = float(alpha if alpha else rank) / rank
    added, skipped, params = 0, [], []
    for name, module in model.named_modules():
        if getattr(module, "sdnq_dequantizer", None) is None or not pick(name):
            continue
        try:
            why = lora_unsupported_reason(module, convs=convs)
        except Exception as e:  # noqa: BLE001  a foreign record the predicate cannot read: leave the layer alone
            why = f"{type(e).__name__} while reading the layer's record: {e}"
        if why is not None:
            skipped.append((name or type(module).__name__, why))
            continue
        dq = module.sdnq_dequantizer
        conv = getattr(dq, "layer_class_name", None) not in linear_types
        if conv:  # PEFT's shapes: lora_A.weight [rank, C_in, *kernel], lora_B.weight [C_out, rank, 1(, 1)]
            shape = tuple(int(d) for d in dq.original_shape)
            n, k = shape[0], math.prod(shape[1:])
            down_shape, up_shape = (rank, *shape[1:]), (n, rank) + (1,) * (len(shape) - 2)
        else:
            n, k = int(dq.out_features), int(dq.in_features)
            down_shape, up_shape = (rank, k), (n, rank)
        pdt = dq.result_dtype if dtype is None else dtype
        dev = module.weight.device
        magnitude = None
        if use_dora:  # the initial magnitude comes from the kernel every forward runs: c == 1.0f exactly until a parameter moves
            magnitude = torch.sqrt(_layer_normsq(module, None, None).detach().to(torch.float32))
            if not bool((magnitude > 0).all()):
                skipped.append((name or type(module).__name__, "DoRA needs a non-zero norm of every weight row (the layer has an all-zero "
                                                                "row: magnitude / norm is undefined there)"))
                continue
        bound = 1.0 / math.sqrt(k)  # kaiming_uniform_(a = sqrt(5)) on fan_in = K (C_in * prod(kernel)): sqrt(6 / ((1 + 5) K))
        down = torch.empty(down_shape, dtype=torch.float32).uniform_(-bound, bound, generator=gen)
        module.lora_down = torch.nn.Parameter(down.to(device=dev, dtype=pdt))
        module.lora_up = torch.nn.Parameter(torch.zeros(up_shape, device=dev, dtype=pdt))
        module.lora_scale = scale
        module.lora_dropout = dropout
        fwd = module.forward_func
        wrap = _with_conv_lora if conv else (_with_dora if use_dora else _with_lora)
        module.forward_func = wrap(getattr(fwd, "_sdnq_inference_forward", None) or fwd, fwd)
        _refresh_compile_plan(module)
        params += [module.lora_down, module.lora_up]
        if use_dora:
            module.lora_magnitude = torch.nn.Parameter(magnitude.to(dev))
            module.lora_dora = True
            params.append(module.lora_magnitude)
        added += 1
    _warn_skipped("add_lora", "SDNQ layer(s) got no adapter", skipped)
    return LoRAResult(added, skipped, params)


def _lora_modules(model: torch.nn.Module):
    for name, module in model.named_modules():
        if getattr(getattr(module, "forward_func", None), "_sdnq_lora_base", None) is not None:
            yield name, module


def _take_off(module) -> bool:
    """One layer's part of `remove_lora`: the forward back, the attributes deleted, the compile plan refreshed.  False: no adapter there."""
    wrapped = getattr(getattr(module, "forward_func", None), "_sdnq_lora_base", None) is not None
    if not wrapped and "lora_down" not in module.__dict__.get("_parameters", {}):
        return False
    if wrapped:
        module.forward_func = module.forward_func._sdnq_lora_previous
        _refresh_compile_plan(module)
    for attr in ("lora_down", "lora_up", "lora_scale", "lora_dropout", "lora_magnitude", "lora_dora"):
        if hasattr(module, attr):
            delattr(module, attr)
    return True


def remove_lora(model: torch.nn.Module) -> int:
    """Take the adapters off: every layer gets back the very forward it had before `add_lora` and loses lora_down, lora_up,
    lora_scale and lora_dropout (a DoRA layer lora_magnitude and lora_dora as well).  A layer whose forward was re-pointed after
    `add_lora` (see there) keeps the forward it has now and loses the attributes.  Returns the number of layers changed."""
    return sum(_take_off(module) for module in list(model.modules()))


_PEFT_PREFIX = "base_model.model."


def lora_state_dict(model: torch.nn.Module) -> dict:
    """The adapters under PEFT's key names: ``<module>.lora_A.weight`` [rank, K] (lora_down) and ``<module>.lora_B.weight`` [N, rank]
    (lora_up) -- on a conv layer [rank, C_in, *kernel] and [C_out, rank, 1(, 1)] -- detached.  alpha is not a tensor: PEFT keeps it in its config, here it is the `alpha` of `add_lora`.
    A DoRA layer adds ``<module>.lora_magnitude_vector.weight`` [N] float32 (lora_magnitude)."""
    sd = {}
    for name, module in _lora_modules(model):
        sd[f"{name}.lora_A.weight"] = module.lora_down.detach()
        sd[f"{name}.lora_B.weight"] = module.lora_up.detach()
        if getattr(module, "lora_dora", False):
            sd[f"{name}.lora_magnitude_vector.weight"] = module.lora_magnitude.detach()
    return sd


def _split_keys(sd: dict, who: str) -> dict:
    """{module name: {"A": lora_A, "B": lora_B, "M": magnitude}} of a PEFT-keyed state dict (the key forms of `load_lora_state_dict`)."""
    import re
    found = {}
    for key, value in sd.items():
        bare = key[len(_PEFT_PREFIX):] if key.startswith(_PEFT_PREFIX) else key
        m = re.fullmatch(r"(.*)\.lora_([AB])(?:\.[^.]+)?\.weight", bare)
        if m is None:  # DoRA's magnitude: .weight, .<adapter>.weight, or the bare .<adapter> of older PEFT files
            mm = re.fullmatch(r"(.*)\.lora_magnitude_vector(?:\.weight|\.[^.]+\.weight|\.[^.]+)", bare)
            if mm is None:
                raise KeyError(f"{who}: {key!r} is not a <module>.lora_A.weight / <module>.lora_B.weight key")
            found.setdefault(mm.group(1), {})["M"] = value
            continue
        found.setdefault(m.group(1), {})[m.group(2)] = value
    return found


def load_lora_state_dict(model: torch.nn.Module, sd: dict) -> int:
    """Copy `sd` (the keys of `lora_state_dict`; a leading ``base_model.model.`` and an adapter name as in ``lora_A.default.weight`` are
    accepted) into the adapters `add_lora` put on `model`.  Every layer with an adapter must find both its keys and every key its layer,
    with the shapes of the registered parameters: KeyError / ValueError otherwise.  A DoRA layer needs its magnitude as well, as
    ``<module>.lora_magnitude_vector.weight``, PEFT's ``lora_magnitude_vector.<adapter>.weight`` or the bare ``lora_magnitude_vector.<adapter>``;
    a magnitude key for a layer without DoRA is a KeyError, as any unknown key.  Returns the number of layers loaded."""
    found = _split_keys(sd, "load_lora_state_dict")
    mods = dict(_lora_modules(model))
    missing = [n for n in found if n not in mods]
    if missing:
        raise KeyError(f"load_lora_state_dict: no adapter on {missing[:4]} (add_lora(model) registers them first)")
    stray = [n for n, got in found.items() if "M" in got and not getattr(mods[n], "lora_dora", False)]
    if stray:
        raise KeyError(f"load_lora_state_dict: a lora_magnitude_vector key for {stray[:4]}, which carry no DoRA magnitude "
                       "(add_lora(model, use_dora=True) registers it)")
    count = 0
    for name, module in mods.items():
        got = found.get(name, {})
        dora = bool(getattr(module, "lora_dora", False))
        if not {"A", "B"} <= set(got):
            raise KeyError(f"load_lora_state_dict: {name} needs both lora_A.weight and lora_B.weight (got {sorted(got)})")
        if dora and "M" not in got:
            raise KeyError(f"load_lora_state_dict: {name} is a DoRA layer and needs lora_magnitude_vector.weight as well (got {sorted(got)})")
        for p, v, what in ((module.lora_down, got["A"], "lora_A"), (module.lora_up, got["B"], "lora_B"),
                           *(((module.lora_magnitude, got["M"], "lora_magnitude_vector"),) if dora else ())):
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"load_lora_state_dict: {name}.{what}.weight has shape {tuple(v.shape)}, the adapter {tuple(p.shape)}")
            with torch.no_grad():
                p.copy_(v)
        count += 1
    return count


# ---- merging an adapter into the stored codes (merge_lora, merge_lora_state_dict) --------------------------------------------------------
_MERGE_FORCE_COMPOSITION = False  # tests: send layers the fused kernel serves through the composition route
_MERGE_FIELDS = ("weight", "scale", "zero_point")


class MergeResult(int):
    """What `merge_lora()` / `merge_lora_state_dict()` return: an int (the number of layers whose codes were rewritten) that also carries
    `.merged` -- their qualified names -- and `.skipped` -- [(qualified module name, reason)] of the layers left as they were."""

    def __new__(cls, merged, skipped):
        r = super().__new__(cls, len(merged))
        r.merged, r.skipped = list(merged), list(skipped)
        return r


def merge_unsupported_reason(module, dora: bool = False) -> str | None:
    """None when an adapter on `module` (an SDNQ layer) can be merged into its codes; otherwise the sentence that says why not.  dora: the
    adapter carries a DoRA magnitude."""
    from .common import linear_types
    dq = module.sdnq_dequantizer
    cls = getattr(dq, "layer_class_name", None)
    if cls not in linear_types:
        return f"{cls}: merging is built for quantized Linear layers (merging conv adapters is not built)"
    fwd = getattr(module, "forward_func", None)
    if getattr(fwd, "_sdnq_lora_base", None) is None:  # no adapter on it: what add_lora would say about the layer
        why = lora_unsupported_reason(module)
        if why is not None:
            return why
    if dora and getattr(module, "svd_up", None) is not None:
        return ("DoRA on a layer with SVD factors: merging it is not built (the row scale c would have to reach svd_up as well as the "
                "codes)")
    return None


def _like(old: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """`values` (the logical shape of `old`) in a new tensor with the shape, stride and dtype of `old`."""
    new = torch.empty_strided(old.size(), old.stride(), dtype=old.dtype, device=old.device)
    if values.dtype != old.dtype and not values.dtype.is_floating_point and values.element_size() == old.element_size():
        values = values.view(old.dtype)  # the same code bits under the layer's integer / float8 spelling
    new.copy_(values)
    return new


def _merge_layer(module, down: torch.Tensor, up: torch.Tensor | None, scale: float, c: torch.Tensor | None) -> str:
    """Rewrite the stored codes, scale and zero point of the Linear `module` as the quantization of c[:, None] * (W + scale * up @ down): W
    the float32 value of the stored codes (for a layer with SVD factors the residual -- the factors stay; for a Hadamard layer the rotated
    weight -- `down` is rotated along K first, ops.hadamard: one more rounding of down to the layer dtype).  down [R, K] / up [N, R]
    contiguous in the layer dtype, R % 8 == 0, or both None with c; c [N] float32 or None.  Returns the route, "fused"
    (ops.merge_lowrank: one launch) or "composed" (ops.dequant to float32, torch.addmm, ops.quantize_weight / quantize_codebook: what the
    kernel reports unsupported -- other group sizes, codebooks -- and ranks above 256).  The quantizer works in float32 and the results
    are cast to the dtypes the module stores afterwards, as the loader does.  The new tensors are installed as NEW parameter objects with
    the shape, stride and dtype of the old ones, all at the end: a failure before leaves the layer as it was.  The layer's kernel state,
    fast-path plan, projection group, slab copy and 4-bit tables rebuild on the changed parameter identity (linear._state)."""
    dq = module.sdnq_dequantizer
    qw = linear._state(module).qw
    n, k = qw.n, qw.k
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    with torch.no_grad():
        if had and down is not None:
            down = ops.hadamard(down, had)
        rank = 0 if up is None else up.shape[1]
        codebook = bool(getattr(dq, "use_codebook", False))
        if ops.merge_lowrank_supported(qw) and rank <= 256 and not _MERGE_FORCE_COMPOSITION:
            route = "fused"
            codes, sc, zp = ops.merge_lowrank(qw, up, down, scale, c, weights_dtype=dq.weights_dtype)
        else:
            route = "composed"
            e = ops.dequant(qw, torch.float32, 0, use_svd=False)
            if up is not None:
                e = torch.addmm(e, up.float(), down.float(), alpha=float(scale))
            if c is not None:
                e = c[:, None] * e
            if codebook:
                codes, sc = ops.quantize_codebook(e, dq.weights_dtype, qw.group_size)
                zp = None
            else:
                codes, sc, zp = ops.quantize_weight(e, dq.weights_dtype, qw.group_size)
        old = {name: _attr(module, name) for name in _MERGE_FIELDS}
        w_old = old["weight"]
        if dq.weight_is_transposed:  # logical [K, N] over the physical [N][K] bytes
            w_new = _like(w_old, codes.reshape(n, k).t())
        else:
            w_new = _like(w_old, codes.reshape(w_old.shape))
        new = {"weight": w_new, "scale": _like(old["scale"], sc.reshape(old["scale"].shape).to(old["scale"].dtype))}
        if old["zero_point"] is not None:
            new["zero_point"] = _like(old["zero_point"], zp.reshape(old["zero_point"].shape).to(old["zero_point"].dtype))
    for name, t in new.items():  # nothing above touched the module
        if name in module._parameters:
            module._parameters[name] = torch.nn.Parameter(t, requires_grad=False)
        elif name in module._buffers:
            module._buffers[name] = t
        else:
            setattr(module, name, t)
    return route


def _warn_skipped(who: str, what: str, skipped) -> None:
    """ONE warning for the layers a public function `who` left alone, attributed to its caller (so `who` calls this itself): their
    number, `what` became of them, and the first eight with their reasons."""
    if skipped:
        import warnings
        warnings.warn(f"sdnq_amd.{who}: {len(skipped)} {what}: "
                      + "; ".join(f"{n} ({w})" for n, w in skipped[:8]) + (" ..." if len(skipped) > 8 else ""), stacklevel=3)


def _merge_operands(module, down: torch.Tensor, up: torch.Tensor, magnitude, scale=None):
    """(down [R', K], up [N, R'], c [N] float32 | None) as _merge_layer takes them: the factors in the layer dtype on the layer's device,
    contiguous, the rank padded to a multiple of 8 (`pad_rank`), and with a DoRA `magnitude` c = magnitude / || W + scale * up @ down ||
    (scale None: the layer's lora_scale), the norm from the very factors that are merged."""
    dt, dev = module.sdnq_dequantizer.result_dtype, module.weight.device
    with torch.no_grad():
        down, up = pad_rank(down.detach().to(device=dev, dtype=dt), up.detach().to(device=dev, dtype=dt))
        c = None
        if magnitude is not None:
            c = (magnitude.detach().to(device=dev, dtype=torch.float32) / torch.sqrt(_layer_normsq(module, down, up, scale))).contiguous()
    return down, up, c


def merge_lora(model: torch.nn.Module, targets=None) -> MergeResult:
    """Fold the adapters `add_lora` put on `model` into the stored codes of their layers (PEFT's ``merge_and_unload``) and take them off:
    afterwards the layer is a plain quantized layer again -- no low-rank launches, no norm launch -- whose weight is the re-quantization
    of W + lora_scale * up @ down (DoRA: of c[:, None] * that, c = lora_magnitude / || W + lora_scale * up @ down ||), and
    ``save_sdnq_model`` writes it as a plain quantized checkpoint.  `targets` selects layers as in `add_lora`.  The factors are taken in
    the layer dtype, as the forward casts them; dropout is ignored (``eval()`` semantics).  Per layer: `_merge_layer`, then what
    `remove_lora` does.  LOSSY: the codes are re-quantized (an error of up to half a step of the NEW scales on top of the adapter's
    effect) and there is no unmerge; keep ``lora_state_dict(model)`` if the adapter is to be used again.  Conv adapters and DoRA on layers
    with SVD factors are not merged: they are listed in ``.skipped`` with one sentence each and in ONE ``warnings.warn``, and keep their
    adapters.  A per-layer error report is not built."""
    pick = _selected(targets)
    merged, skipped = [], []
    for name, module in list(_lora_modules(model)):
        if not pick(name):
            continue
        dora = bool(getattr(module, "lora_dora", False))
        why = merge_unsupported_reason(module, dora)
        if why is not None:
            skipped.append((name or type(module).__name__, why))
            continue
        down, up, c = _merge_operands(module, _attr(module, "lora_down"), _attr(module, "lora_up"),
                                      _attr(module, "lora_magnitude") if dora else None)
        _merge_layer(module, down, up, float(module.lora_scale), c)
        _take_off(module)
        merged.append(name or type(module).__name__)
    _warn_skipped("merge_lora", "layer(s) were not merged", skipped)
    return MergeResult(merged, skipped)


def pad_rank(down: torch.Tensor, up: torch.Tensor):
    """(down [R', K], up [N, R']) with R' the next multiple of 8 (at least 8): zero rows of down, zero columns of up -- the same product."""
    r = down.shape[0]
    r8 = max(8, -(-r // 8) * 8)
    if r8 == r:
        return down.contiguous(), up.contiguous()
    d = down.new_zeros((r8, down.shape[1]))
    u = up.new_zeros((up.shape[0], r8))
    d[:r] = down
    u[:, :r] = up
    return d, u


def merge_lora_state_dict(model: torch.nn.Module, sd: dict, scale: float = 1.0) -> MergeResult:
    """Apply a PEFT-keyed LoRA file to a quantized `model` that carries NO adapters: every ``<module>.lora_A.weight`` [r, K] /
    ``<module>.lora_B.weight`` [N, r] pair of `sd` (the key forms of `load_lora_state_dict`) is folded into the codes of its layer as
    W + scale * B @ A -- the caller computes ``scale = alpha / r`` (alpha is not in the file).  The rank is read from the tensors; one that
    is no multiple of 8 is padded with zero rows / columns (`pad_rank`).  A ``lora_magnitude_vector`` key makes the layer's merge DoRA's.
    The factors are cast to the layer dtype.  KeyError: a key that names no quantized layer of `model`, or a layer with one factor only;
    ValueError: a factor of the wrong shape, or a layer that carries an adapter (``merge_lora`` merges those).  Everything is checked
    before the first layer changes.  Conv layers, float32 layers, layers that do not run on the MI355X forwards and DoRA on layers with
    SVD factors are listed in ``.skipped`` (ONE warning) and left alone.  Lossy, no unmerge: see `merge_lora`."""
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"merge_lora_state_dict: scale must be finite (got {scale})")
    found = _split_keys(sd, "merge_lora_state_dict")
    mods = {n: m for n, m in model.named_modules() if getattr(m, "sdnq_dequantizer", None) is not None}
    missing = [n for n in found if n not in mods]
    if missing:
        raise KeyError(f"merge_lora_state_dict: {missing[:4]} name no quantized layer of the model")
    work, skipped = [], []
    for name, got in found.items():
        module = mods[name]
        if not {"A", "B"} <= set(got):
            raise KeyError(f"merge_lora_state_dict: {name} needs both lora_A.weight and lora_B.weight (got {sorted(got)})")
        if getattr(getattr(module, "forward_func", None), "_sdnq_lora_base", None) is not None:
            raise ValueError(f"merge_lora_state_dict: {name} carries an adapter (merge_lora(model) merges the adapters add_lora put on; "
                             "remove_lora(model) takes them off)")
        why = merge_unsupported_reason(module, "M" in got)
        if why is not None:
            skipped.append((name, why))
            continue
        dq = module.sdnq_dequantizer
        n, k = int(dq.out_features), int(dq.in_features)
        a, b = got["A"], got["B"]
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != k or b.shape[0] != n or a.shape[0] != b.shape[1] or a.shape[0] < 1:
            raise ValueError(f"merge_lora_state_dict: {name} needs lora_A [r, {k}] and lora_B [{n}, r] (got {tuple(a.shape)}, {tuple(b.shape)})")
        if "M" in got and tuple(got["M"].shape) != (n,):
            raise ValueError(f"merge_lora_state_dict: {name}.lora_magnitude_vector has shape {tuple(got['M'].shape)}, the layer {n} rows")
        work.append((name, module, a, b, got.get("M")))
    merged = []
    for name, module, a, b, mag in work:
        down, up, c = _merge_operands(module, a, b, mag, scale)
        _merge_layer(module, down, up, scale, c)
        merged.append(name)
    _warn_skipped("merge_lora_state_dict", "layer(s) were not merged", skipped)
    return MergeResult(merged, skipped)
