"""Load-time quantization helpers (host side, torch ops) -- SURVEY 8(f) rank 1.

These run once when a float layer is quantized by this package (benchmarks, tests, users without
pre-quantized checkpoints); they are not on the per-forward hot path.  Semantics follow the reference's
quant_utils.py (get_scale_symmetric :23-24, get_scale_asymmetric :10-19, quantize_weight :28-56,
apply_svdquant :124-141, build_hadamard :145-175, get_hadamard_group_size :212-218).
"""
from __future__ import annotations

import torch

from .common import dtype_dict

_H4 = ((1, 1, 1, -1), (1, 1, -1, 1), (1, -1, 1, 1), (-1, 1, 1, 1))
_H2 = ((1, 1), (1, -1))
_HADAMARD_CACHE: dict = {}


def is_pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


def is_pow4(n: int) -> bool:
    return is_pow2(n) and (n.bit_length() & 1) == 1


def get_hadamard(n: int, dtype: torch.dtype = torch.float32, device=None) -> torch.Tensor:
    """H_n = kron powers of H4 (n a power of 4) or of Sylvester's H2, divided by sqrt(n) in ``dtype``."""
    key = (n, dtype, str(device))
    h = _HADAMARD_CACHE.get(key)
    if h is None:
        if not is_pow2(n):
            raise RuntimeError(f"Hadamard Group Size must be a power of 2 but got {n}.")
        base = torch.tensor(_H4 if is_pow4(n) else _H2, dtype=dtype, device=device)
        h = base
        while h.shape[0] < n:
            h = torch.kron(h, base)
        h = h.div_(n ** 0.5)
        _HADAMARD_CACHE[key] = h
    return h


def get_hadamard_group_size(channel_size: int, group_size: int) -> tuple[bool, int]:
    g = 1
    while g < min(channel_size, group_size):
        g *= 2
    while channel_size % g != 0:
        g //= 2
    return g >= 4, g


def rotate_hadamard(weight: torch.Tensor, group_size: int) -> torch.Tensor:
    """weight.view(..., K/g, g) @ H_g  (load-time, on the float weight)."""
    h = get_hadamard(group_size, dtype=weight.dtype, device=weight.device)
    return torch.matmul(weight.unflatten(-1, (-1, group_size)), h).flatten(-2, -1)


def apply_hadamard(weight: torch.Tensor, group_size: int = 256, is_conv: bool = False):
    """quant_utils.py:222-236.  Conv weights ([C_out, C_in, *kernel], or already flattened for the direct matmul): the group size is
    chosen from dimension 1 and the groups run along the flattened (C_in, kernel) axis."""
    use, g = get_hadamard_group_size(weight.shape[1] if is_conv else weight.shape[-1], group_size)
    if use:
        if is_conv and weight.ndim > 2:
            weight = rotate_hadamard(weight.flatten(1, -1), g).unflatten(-1, tuple(weight.shape[1:]))
        else:
            weight = rotate_hadamard(weight, g)
    return weight, use, g


def apply_svdquant(weight: torch.Tensor, rank: int = 32, steps: int = 8, dtype: torch.dtype | None = None):
    """Split W = svd_up @ svd_down + residual with a randomized low-rank SVD; the residual is what gets quantized."""
    shape = weight.shape
    if weight.ndim > 2:  # conv weights: factor the flattened [C_out, C_in * kernel] matrix (quant_utils.py:126-129)
        weight = weight.flatten(1, -1)
    w = weight.to(torch.float32) if weight.dtype != torch.float64 else weight
    u, s, v = torch.svd_lowrank(w, q=rank, niter=steps)
    svd_up = u * s.unsqueeze(0)
    svd_down = v.t()
    if dtype is not None:
        svd_up, svd_down = svd_up.to(dtype), svd_down.to(dtype)
    residual = w - torch.mm(svd_up, svd_down)
    if len(shape) > 2:
        residual = residual.unflatten(-1, tuple(shape[1:]))
    return residual, svd_up, svd_down


def quantize_weight(weight: torch.Tensor, dim, weights_dtype: str, dtype: torch.dtype | None = None):
    """-> (quantized values in the dtype's torch_dtype, scale, zero_point | None)."""
    ent = dtype_dict[weights_dtype]
    w = weight if weight.dtype == torch.float64 else weight.to(torch.float32)
    if ent["is_unsigned"]:
        lo = torch.amin(w, dim=dim, keepdim=True)
        hi = torch.amax(w, dim=dim, keepdim=True)
        scale = (hi - lo) / (ent["max"] - ent["min"])
        zero_point = lo if ent["min"] == 0 else lo - scale * ent["min"]
        if dtype is not None:
            scale, zero_point = scale.to(dtype), zero_point.to(dtype)
        q = (w - zero_point) / scale
    else:
        scale = torch.amax(w.abs(), dim=dim, keepdim=True) / ent["max"]
        zero_point = None
        if dtype is not None:
            scale = scale.to(dtype)
        q = w / scale
    if ent["is_integer"]:
        q = q.round_()
    else:
        q = q.nan_to_num_()
    q = q.clamp_(ent["min"], ent["max"]).to(ent["torch_dtype"])
    return q, scale, zero_point


def dequantize_host(dq, weight: torch.Tensor, scale: torch.Tensor, zero_point=None, svd_up=None, svd_down=None,
                    dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Torch restatement of SDNQDequantizer.__call__(..., skip_quantized_matmul=dq.use_quantized_matmul, dtype=dtype) for host tensors
    (the reference's dequantize_weight, dequantizer.py:135-162, with dequantize_symmetric / _asymmetric / _codebook :15-131): the
    dynamic search's loss of a candidate on the CPU.  The HIP path computes the same quantity without the copy (ops.dequant_loss_sum)."""
    from . import packed
    ent = dtype_dict[dq.weights_dtype]
    shape = dq.quantized_weight_shape
    if ent["is_packed"]:
        if ent["is_integer"]:
            w = packed.unpack_int(weight, dq.weights_dtype, shape, dtype=torch.int32 if dq.use_codebook else scale.dtype)
        else:
            w = packed.unpack_float(weight, dq.weights_dtype, shape)
    else:
        w = weight
    if dq.use_codebook:
        if dq.group_size == -2:
            r = scale[w.to(torch.int32)]
        else:
            r = scale.gather((2 if dq.group_size != -1 else 1) if dq.is_conv else -1, w.to(torch.int64))
    elif ent["is_unsigned"]:
        r = torch.addcmul(zero_point, w.to(scale.dtype), scale)
    else:
        r = w.to(scale.dtype) * scale  # (out of place: a native float16 code tensor would be its own .to(float16))
    if dq.weight_is_transposed:
        r = r.t()
    if dq.result_shape is not None:
        r = r.reshape(dq.result_shape)
    is_conv = r.ndim > 2 and w.ndim > 2
    if svd_up is not None:
        if dq.use_quantized_matmul:
            svd_up, svd_down = svd_up.t().contiguous(), svd_down.contiguous().t()
        if is_conv:
            r = r + torch.mm(svd_up, svd_down).unflatten(-1, tuple(r.shape[1:]))
        else:
            r = r.to(svd_up.dtype).addmm_(svd_up, svd_down)
    r = r.to(dtype)
    if dq.use_hadamard:
        g = dq.hadamard_group_size
        h = get_hadamard(g, dtype=dtype, device=r.device)
        if is_conv:
            r = torch.matmul(r.flatten(1, -1).unflatten(-1, (-1, g)), h).flatten(-2, -1).unflatten(-1, tuple(r.shape[1:]))
        else:
            r = torch.matmul(r.unflatten(-1, (-1, g)), h).flatten(-2, -1)
    return r


def _lloyd_max_rows(x: torch.Tensor, n_levels: int, steps: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Lloyd-Max levels of every row of a float32 [R, S] matrix -> (codes int64 [R, S], sorted levels float32 [R, L]).

    Starts from L evenly spaced levels between the row's min and max (one fused multiply-add each), then `steps` rounds of:
    sort, assign every value to the level whose midpoint interval holds it (a value on a midpoint takes the lower level), move
    every occupied level to the mean of its members.  On CPU tensors `scatter_add_` adds each level's members in element order,
    which is the reference's rounding."""
    lo, hi = torch.aminmax(x, dim=-1, keepdim=True)
    step = (hi - lo) / (n_levels - 1)
    idx = torch.arange(n_levels, dtype=x.dtype, device=x.device)
    levels = torch.addcmul(lo, idx, step)
    ones = torch.ones(x.shape, dtype=torch.int32, device=x.device)

    def assign(lv):
        mids = (lv[:, 1:] + lv[:, :-1]) * 0.5
        return torch.searchsorted(mids, x)

    for _ in range(steps):
        levels = torch.sort(levels, dim=-1).values
        codes = assign(levels)
        count = torch.zeros(levels.shape, dtype=torch.int32, device=x.device).scatter_add_(1, codes, ones)
        total = torch.zeros_like(levels).scatter_add_(1, codes, x)
        levels = torch.where(count > 0, total / count.clamp(min=1), levels)
    levels = torch.sort(levels, dim=-1).values
    return assign(levels), levels


def quantize_codebook(weight: torch.Tensor, dim: int, weights_dtype: str, steps: int = 24, dtype: torch.dtype | None = None):
    """Codebook quantization along `dim` (the reference's use_codebook): -> (codes of weight's shape in the dtype's torch type,
    levels).  The levels take weight's shape with `dim` replaced by the L = 2^bits level axis: [N, L] / [N, G, L] for Linear and
    embedding tables, [N, L, *kernel] / [N, G, L, *kernel] for conv weights.  `dtype`: the scale dtype the levels are cast to last.
    Meta tensors give placeholders of those shapes."""
    ent = dtype_dict[weights_dtype]
    if not (ent["is_integer"] and ent["is_unsigned"]):
        raise NotImplementedError("codebook quantization is only supported with unsigned integer dtypes")
    n_levels = int(ent["max"]) + 1
    dim = dim % weight.dim()
    lshape = list(weight.shape)
    lshape[dim] = n_levels
    if weight.is_meta:
        return (torch.empty(weight.shape, dtype=ent["torch_dtype"], device="meta"),
                torch.empty(lshape, dtype=dtype or torch.float32, device="meta"))
    x = weight.to(torch.float32).movedim(dim, -1)
    moved = x.shape
    codes, levels = _lloyd_max_rows(x.reshape(-1, moved[-1]).contiguous(), n_levels, steps)
    codes = codes.view(moved).movedim(-1, dim)
    levels = levels.view(*moved[:-1], n_levels).movedim(-1, dim).contiguous()
    if dtype is not None:
        levels = levels.to(dtype)
    return codes.to(ent["torch_dtype"]).contiguous(), levels
