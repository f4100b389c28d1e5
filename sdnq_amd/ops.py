"""Tensor-level wrappers over the C ABI (``include/sdnq_hip.h``).

PyTorch is only plumbing here: it owns device memory and the current HIP stream; every arithmetic
step runs in the hand-written gfx950 kernels of ``libsdnq_hip.so``.  All functions raise
``SdnqHipError`` on a non-zero status -- there is no eager fallback.
"""
from __future__ import annotations

import ctypes
import os
import typing
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import BF16, F16, F32, MM_FP8, MM_I8, SdnqWeight, check
from .common import dtype_dict

_FLOAT_CODE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_MM_TORCH = {MM_I8: torch.int8, MM_FP8: torch.float8_e4m3fn}


def float_code(dt: torch.dtype) -> int:
    try:
        return _FLOAT_CODE[dt]
    except KeyError:
        raise _lib.SdnqHipError(f"unsupported float dtype {dt}") from None


def mm_code(matmul_dtype: str) -> int:
    if matmul_dtype == "int8":
        return MM_I8
    if matmul_dtype in ("fp8", "float8_e4m3fn"):
        return MM_FP8
    raise _lib.SdnqHipError(f"unsupported quantized_matmul_dtype {matmul_dtype!r}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor) -> int:
    """Raw handle of torch's current HIP stream on t's device (the C accessor is ~10x cheaper than torch.cuda.current_stream,
    which dominated the host cost of an eager step)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SdnqHipError("sdnq_amd kernels need tensors on a gfx950 device (got a CPU tensor); "
                                    "there is no CPU fallback in the product path")


# ---------------------------------------------------------------------------------------------
# quantized weight descriptor
# ---------------------------------------------------------------------------------------------
@dataclass
class QuantWeight:
    """A quantized Linear weight in the physical layout the kernels read ([N][K], scales [N][G])."""
    desc: SdnqWeight
    n: int
    k: int
    group_size: int
    keep: tuple  # tensors kept alive for the raw pointers in `desc`
    scale_dtype: torch.dtype = torch.float32  # dtype the LAYER stores scale / zero_point in (dequantize_fp32=False: the model dtype)


def _storage_kind(weights_dtype: str):
    ent = dtype_dict[weights_dtype]
    bits = ent["num_bits"]
    native = 0
    if ent["is_integer"]:
        kind = _lib.KIND_UINT if ent["is_unsigned"] else _lib.KIND_INT
        if ent["is_packed"]:
            storage = _lib.ST_PACKED_U8 if bits < 8 else _lib.ST_PACKED_I16
        elif bits == 8:
            storage = _lib.ST_RAW8
        elif bits == 16:
            storage = _lib.ST_RAW16
        else:
            raise _lib.SdnqHipError(f"weights_dtype {weights_dtype} is not a storage format of the matmul path")
    else:
        kind = _lib.KIND_UFLOAT if ent["is_unsigned"] else _lib.KIND_FLOAT
        if ent["is_packed"]:
            storage = _lib.ST_RAW8 if bits == 8 else (_lib.ST_RAW16 if bits == 16 else (_lib.ST_PACKED_U8 if bits < 8 else _lib.ST_PACKED_I16))
        else:
            native = 1
            if bits == 8:
                storage = _lib.ST_RAW8
            elif bits == 16:
                storage = _lib.ST_RAW16
            else:
                raise _lib.SdnqHipError(f"weights_dtype {weights_dtype} is not a storage format of the matmul path")
    return storage, kind, bits, ent["exponent"], ent["mantissa"], native


def make_quant_weight(weights_dtype: str, weight: torch.Tensor, scale: torch.Tensor, zero_point, svd_up, svd_down,
                      n: int, k: int, group_size: int, transposed: bool, svd_transposed: bool | None = None,
                      positions: int = 1, codebook: bool = False) -> QuantWeight:
    """Canonicalise module tensors (reference layouts) into the kernels' physical layout.

    transposed=False: weight is packed bytes / [N,K] / [N,G,g] (element order [N][K]); svd_up [N,R], svd_down [R,K].
    transposed=True : the qmm layout the reference's quantizer produces when use_quantized_matmul and not
                      re_quantize_for_matmul and not packed (quantizer.py:228-244): weight logical [K,N] with
                      strides (1,K) -- the same bytes as physical [N][K]; a *contiguous* [K,N] (as stored in
                      safetensors) is re-laid out once, like prepare_weight_for_matmul (quant_utils.py:240-249);
                      scale [1,N].
    svd_transposed  : svd_up [R,N], svd_down [K,R] -- the quantizer transposes the SVD factors whenever
                      use_quantized_matmul is on, independent of the weight layout (quantizer.py:164-167).
    positions       : P > 1 for conv weights [N, C_in, *kernel] quantized along C_in (quantizer.py:120-123, 205-209):
                      k = C_in * P, group_size counts channels, scale / zero_point hold N * (C_in / group_size) * P values.
    codebook        : `scale` is the level table of a use_codebook layer, 2^bits levels per (row, group[, position]) with the level
                      axis before the kernel positions ([N, L], [N, G, L], [N, L, *kernel], [N, G, L, *kernel]); no zero point.
    """
    if svd_transposed is None:
        svd_transposed = transposed
    _require_cuda(weight, scale)
    storage, kind, bits, ebits, mbits, native = _storage_kind(weights_dtype)
    levels = 1
    if codebook:
        if kind != _lib.KIND_UINT or bits > 8 or transposed or zero_point is not None:
            raise _lib.SdnqHipError(f"codebook weights are unsigned integer codes of up to 8 bits without a zero point (got {weights_dtype})")
        kind, levels = _lib.KIND_CODEBOOK, 1 << bits
    if transposed:
        if tuple(weight.shape) != (k, n):
            raise _lib.SdnqHipError(f"transposed weight must be [K,N]=({k},{n}), got {tuple(weight.shape)}")
        w_phys = weight.t()
        if not w_phys.is_contiguous():
            w_phys = w_phys.contiguous()
    else:
        w_phys = weight if weight.is_contiguous() else weight.contiguous()
        if w_phys.dtype in (torch.int64, torch.bool):
            # 1-bit types: the reference's pack_uint1 on a bool tensor promotes to int64 words holding 8 bits each
            # (packed_int/pack.py:309-321); the kernels read uint8 words
            w_phys = w_phys.to(torch.uint8)
    scale_dtype = scale.dtype
    if scale_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise _lib.SdnqHipError(f"scale must be float32, bfloat16 or float16, got {scale_dtype}")
    if scale_dtype != torch.float32 and bits > 8:
        raise _lib.SdnqHipError("16-bit scales with formats wider than 8 bits are not built (the codes are not exact in the scale dtype)")
    if zero_point is not None and zero_point.dtype != scale_dtype:
        raise _lib.SdnqHipError("scale and zero_point must share one dtype (loader.py:277-280 casts both)")
    g = (k // positions) // group_size * positions
    # dequantize_fp32=False keeps scale / zero_point in the model dtype (quantizer.py:147-156); the kernels read the exact float32
    # upcast and SdnqWeight.scale_dtype tells them where the reference's 16-bit tensors round
    sc = scale.to(torch.float32).contiguous().view(-1)
    if sc.numel() != n * g * levels:
        raise _lib.SdnqHipError(f"scale has {sc.numel()} elements, expected N*G{'*L' if codebook else ''} = {n * g * levels}")
    zp = None
    if zero_point is not None:
        zp = zero_point.to(torch.float32).contiguous().view(-1)
        if zp.numel() != n * g:
            raise _lib.SdnqHipError("zero_point size mismatch")
    up = down = None
    rank, svd_dt = 0, 0
    if svd_up is not None:
        if svd_transposed:  # [R,N] , [K,R]
            up = svd_up.t().contiguous()
            down = svd_down.t().contiguous()
        else:  # [N,R] , [R,K]
            up = svd_up.contiguous()
            down = svd_down.contiguous()
        rank = up.shape[1]
        svd_dt = float_code(up.dtype)
    d = SdnqWeight(weight=_ptr(w_phys), scale=_ptr(sc), zero_point=_ptr(zp), svd_up=_ptr(up), svd_down=_ptr(down),
                   n=n, k=k, group_size=group_size, svd_rank=rank, svd_dtype=svd_dt, storage=storage, kind=kind,
                   bits=bits, exponent=ebits, mantissa=mbits, native_float=native, positions=positions,
                   scale_dtype=float_code(scale_dtype))
    return QuantWeight(desc=d, n=n, k=k, group_size=group_size, keep=(w_phys, sc, zp, up, down), scale_dtype=scale_dtype)


# ---------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------
def rowquant(x2d: torch.Tensor, mm: int, hadamard_group: int = 0, want_rowsum: bool = False, want_xrot: bool = False,
             prefetch: torch.Tensor | None = None, asymmetric: bool = False):
    """Row-quantize activations [M,K] -> (xq [M,K] int8|fp8, xs [M,1] f32, rowsum [M] i32|None, xrot|None).
    `prefetch`: tensor (the weight operand of the following matmul) to pull into the last-level cache meanwhile.
    `asymmetric`: int8 activations with a zero point (uint8 matmul); returns a 5th value xzp [M] f32."""
    _require_cuda(x2d)
    assert x2d.ndim == 2 and x2d.stride(1) == 1
    m, k = x2d.shape
    xq = torch.empty((m, k), device=x2d.device, dtype=_MM_TORCH[mm])
    xs = torch.empty((m, 1), device=x2d.device, dtype=torch.float32)
    rowsum = torch.empty((m,), device=x2d.device, dtype=torch.int32) if want_rowsum else None
    # rows beyond the kernel's register cache (K > 5120) are rotated once into this buffer and quantized from it, so it is
    # allocated for them even when the caller does not want the rotated copy
    # (group 256 on 16-bit activations up to K = 16384 rotates on the matrix cores, whole row in registers: no scratch copy)
    mfma_rot = hadamard_group == 256 and x2d.dtype != torch.float32 and k <= 16384 and not asymmetric
    need_rot = bool(hadamard_group) and (want_xrot or (k > 5120 and not mfma_rot))
    xrot = torch.empty((m, k), device=x2d.device, dtype=x2d.dtype) if need_rot else None
    xzp = torch.empty((m,), device=x2d.device, dtype=torch.float32) if asymmetric else None
    check(_lib.load().sdnq_hip_rowquant(x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), mm, hadamard_group,
                                        xq.data_ptr(), xs.data_ptr(), _ptr(rowsum), _ptr(xrot), _ptr(prefetch),
                                        0 if prefetch is None else prefetch.numel() * prefetch.element_size(), _ptr(xzp),
                                        _stream(x2d)), "rowquant")
    if not want_xrot:
        xrot = None  # scratch only: released here (stream-ordered reuse by the caching allocator)
    if asymmetric:
        return xq, xs, rowsum, xrot, xzp
    return xq, xs, rowsum, xrot


def colquant_t(x2d: torch.Tensor, want_colsum: bool = False):
    """sdnq_hip_colquant_t: int8-quantize x2d [R,C] per COLUMN and return the codes transposed -- (xq_t [C, ld_t] int8 with
    ld_t = R rounded up to 16 and columns [R, ld_t) zero, xs [C,1] f32, colsum [C] f32 | None): the operand of a scaled matmul that
    reduces over the rows of x2d (the int8 training Linear's grad_input and grad_weight)."""
    _require_cuda(x2d)
    assert x2d.ndim == 2 and x2d.stride(1) == 1
    r, c = x2d.shape
    lib = _lib.load()
    nbytes = lib.sdnq_hip_colquant_t_workspace_bytes(r, c)
    if nbytes < 0:
        check(int(nbytes), "colquant_t")
    ld_t = (r + 15) // 16 * 16
    xq_t = torch.empty((c, ld_t), device=x2d.device, dtype=torch.int8)
    xs = torch.empty((c, 1), device=x2d.device, dtype=torch.float32)
    colsum = torch.empty((c,), device=x2d.device, dtype=torch.float32) if want_colsum else None
    ws = torch.empty((nbytes,), device=x2d.device, dtype=torch.uint8)  # stream-ordered reuse by the caching allocator
    check(lib.sdnq_hip_colquant_t(x2d.data_ptr(), float_code(x2d.dtype), r, c, x2d.stride(0), xq_t.data_ptr(), ld_t, xs.data_ptr(),
                                  _ptr(colsum), ws.data_ptr(), nbytes, _stream(x2d)), "colquant_t")
    return xq_t, xs, colsum


def rowquant_lp(x2d: torch.Tensor, mm: int, hadamard_group: int = 0, want_rowsum: bool = False, want_xrot: bool = False):
    """sdnq_hip_rowquant_lp: the activation quantization carried out in x2d's own 16-bit dtype (dequantize_fp32=False layers).
    Returns (xq, xs [M,1] f32 holding dtype-representable values, rowsum | None, xrot | None)."""
    _require_cuda(x2d)
    assert x2d.ndim == 2 and x2d.stride(1) == 1 and x2d.dtype in (torch.bfloat16, torch.float16)
    m, k = x2d.shape
    xq = torch.empty((m, k), device=x2d.device, dtype=_MM_TORCH[mm])
    xs = torch.empty((m, 1), device=x2d.device, dtype=torch.float32)
    rowsum = torch.empty((m,), device=x2d.device, dtype=torch.int32) if want_rowsum else None
    xrot = torch.empty((m, k), device=x2d.device, dtype=x2d.dtype) if (hadamard_group and want_xrot) else None
    check(_lib.load().sdnq_hip_rowquant_lp(x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), mm, hadamard_group,
                                           xq.data_ptr(), xs.data_ptr(), _ptr(rowsum), _ptr(xrot), _stream(x2d)), "rowquant_lp")
    return xq, xs, rowsum, xrot


def rowquant_lp_asym(x2d: torch.Tensor, hadamard_group: int = 0, want_rowsum: bool = False, want_xrot: bool = False):
    """sdnq_hip_rowquant_lp_asym: quantize_uint_mm_input in x2d's own 16-bit dtype (the uint8 matmul of dequantize_fp32=False layers).
    Returns (xq int8, xs [M,1] f32, xzp [M] f32 -- both holding dtype-representable values --, rowsum | None, xrot | None: the rotated
    activation of a Hadamard layer, for its SVD product)."""
    _require_cuda(x2d)
    assert x2d.ndim == 2 and x2d.stride(1) == 1 and x2d.dtype in (torch.bfloat16, torch.float16)
    m, k = x2d.shape
    xq = torch.empty((m, k), device=x2d.device, dtype=torch.int8)
    xs = torch.empty((m, 1), device=x2d.device, dtype=torch.float32)
    xzp = torch.empty((m,), device=x2d.device, dtype=torch.float32)
    rowsum = torch.empty((m,), device=x2d.device, dtype=torch.int32) if want_rowsum else None
    xrot = torch.empty((m, k), device=x2d.device, dtype=x2d.dtype) if (want_xrot and hadamard_group) else None
    check(_lib.load().sdnq_hip_rowquant_lp_asym(x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), hadamard_group, xq.data_ptr(),
                                                xs.data_ptr(), xzp.data_ptr(), _ptr(rowsum), _ptr(xrot), _stream(x2d)), "rowquant_lp_asym")
    return xq, xs, xzp, rowsum, xrot


def scaled_mm_lp_uzp(a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, rowsum, zp, a_zp: torch.Tensor,
                     w_colsum_scaled: torch.Tensor, zp_k: int = 0, t=None, svd_up=None) -> torch.Tensor:
    """sdnq_hip_scaled_mm_lp_uzp[_svd]: the uint8 matmul's epilogue on bfloat16 tensors (see the header); t [M,R] / svd_up [N,R] bf16 add the
    low-rank product to the bias (layers with SVD factors).  Returns [M,N] bf16."""
    _require_cuda(a, b_phys, sa, sb, bias, rowsum, zp, a_zp, w_colsum_scaled, t, svd_up)
    m, k = a.shape
    n = b_phys.shape[0]
    if bias is not None and bias.dtype != torch.bfloat16:
        raise _lib.SdnqHipError("scaled_mm_lp_uzp: bias must be bfloat16")
    out = torch.empty((m, n), device=a.device, dtype=torch.bfloat16)
    f32 = lambda t: None if t is None else t.reshape(-1).to(torch.float32).contiguous()  # noqa: E731
    sa_, sb_, zp_, azp_, wcs_ = f32(sa), f32(sb), f32(zp), f32(a_zp), f32(w_colsum_scaled)
    if t is not None:
        if t.dtype != torch.bfloat16 or svd_up.dtype != torch.bfloat16:
            raise _lib.SdnqHipError("scaled_mm_lp_uzp: low-rank factors must be bfloat16")
        t, svd_up = t.contiguous(), svd_up.contiguous()
        check(_lib.load().sdnq_hip_scaled_mm_lp_uzp_svd(a.data_ptr(), b_phys.data_ptr(), sa_.data_ptr(), sb_.data_ptr(), _ptr(None if bias is None else bias.contiguous()),
                                                        _ptr(rowsum), _ptr(zp_), azp_.data_ptr(), wcs_.data_ptr(), zp_k, t.data_ptr(), svd_up.data_ptr(),
                                                        t.shape[1], out.data_ptr(), m, n, k, _stream(a)), "scaled_mm_lp_uzp_svd")
        return out
    check(_lib.load().sdnq_hip_scaled_mm_lp_uzp(a.data_ptr(), b_phys.data_ptr(), sa_.data_ptr(), sb_.data_ptr(), _ptr(None if bias is None else bias.contiguous()),
                                                _ptr(rowsum), _ptr(zp_), azp_.data_ptr(), wcs_.data_ptr(), zp_k, out.data_ptr(), m, n, k, _stream(a)),
          "scaled_mm_lp_uzp")
    return out


def scaled_mm_lp(mm: int, a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, t=None, svd_up=None,
                 rowsum=None, zp=None):
    """sdnq_hip_scaled_mm_lp[_zp]: the scaled matmul of bfloat16-scale layers (accumulator, activation-scale product and result each
    rounded to bf16); bias None | [N] | [M,N] bf16; t [M,R] / svd_up [N,R] bf16 add the low-rank bias; rowsum [M] i32 + zp [N] f32
    (bf16-representable) the zero-point term of unsigned weights.  Returns [M,N] bf16."""
    _require_cuda(a, b_phys, sa, sb, bias, t, svd_up, rowsum, zp)
    m, k = a.shape
    n = b_phys.shape[0]
    out = torch.empty((m, n), device=a.device, dtype=torch.bfloat16)
    bias_ndim, ld_bias = 0, 0
    if bias is not None:
        if bias.dtype != torch.bfloat16:
            raise _lib.SdnqHipError("scaled_mm_lp: bias must be bfloat16")
        bias = bias.contiguous()
        bias_ndim, ld_bias = bias.ndim, bias.shape[-1]
    rank = 0
    if t is not None:
        if t.dtype != torch.bfloat16 or svd_up.dtype != torch.bfloat16:
            raise _lib.SdnqHipError("scaled_mm_lp: low-rank factors must be bfloat16")
        t, svd_up = t.contiguous(), svd_up.contiguous()
        rank = t.shape[1]
    if zp is not None:
        zp = zp.reshape(-1).contiguous()
        assert zp.dtype == torch.float32 and rowsum is not None and rowsum.dtype == torch.int32
    check(_lib.load().sdnq_hip_scaled_mm_lp_zp(mm, a.data_ptr(), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias), bias_ndim,
                                               ld_bias, _ptr(t), _ptr(svd_up), rank, _ptr(rowsum if zp is not None else None), _ptr(zp),
                                               out.data_ptr(), m, n, k, _stream(a)), "scaled_mm_lp")
    return out


def scaled_mm(mm: int, a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype):
    """out[M,N] = cast(fma(f32(a @ b_phys^T) * sa, sb, bias)); b_phys is physical [N,K]."""
    _require_cuda(a, b_phys, sa, sb, bias)
    m, k = a.shape
    n = b_phys.shape[0]
    out = torch.empty((m, n), device=a.device, dtype=out_dtype)
    bias_ndim, ld_bias, bias_dt = 0, 0, 0
    if bias is not None:
        bias = bias.contiguous()
        bias_ndim = bias.ndim
        ld_bias = bias.shape[-1]
        bias_dt = float_code(bias.dtype)
    check(_lib.load().sdnq_hip_scaled_mm(mm, a.data_ptr(), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias),
                                         bias_dt, bias_ndim, ld_bias, out.data_ptr(), float_code(out_dtype), m, n, k,
                                         _stream(a)), "scaled_mm")
    return out


def scaled_mm_multi(mm: int, a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype,
                    n_outs: int):
    """One scaled matmul over the stacked weights of `n_outs` layers, each layer's output in its own contiguous [M, N / n_outs]
    tensor (sdnq_hip_scaled_mm_multi)."""
    _require_cuda(a, b_phys)
    m, k = a.shape
    n = b_phys.shape[0]
    seg = n // n_outs
    outs = [torch.empty((m, seg), device=a.device, dtype=out_dtype) for _ in range(n_outs)]
    ptrs = (ctypes.c_void_p * n_outs)(*[o.data_ptr() for o in outs])
    check(_lib.load().sdnq_hip_scaled_mm_multi(mm, a.data_ptr(), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias),
                                               float_code(bias.dtype) if bias is not None else 0, ptrs, n_outs, seg, float_code(out_dtype),
                                               m, n, k, _stream(a)), "scaled_mm_multi")
    return outs


class GemmGroup:
    """Device-resident unit table of a grouped scaled matmul (sdnq_hip_scaled_mm_grouped): the output channels of several layers
    that consume ONE activation, cut into units of `unit_n` channels that point at the layers' own weight / scale / bias tensors
    (no stacked copy).  `members`: [(wq [N_i, K] int8 | fp8 physical, ws [N_i] f32, bias [N_i] | None)], all with one K."""

    def __init__(self, members):
        import math
        import numpy as np
        ns = [int(w.shape[0]) for (w, _, _) in members]
        unit = 0
        for n in ns:
            unit = math.gcd(unit, n)
        if unit % 64:
            raise _lib.SdnqHipError(f"grouped matmul needs layer widths with a common divisor that is a multiple of 64 (got {ns})")
        while unit > 2048 and unit % 128 == 0:  # keep units tile-sized multiples; any divisor of the gcd works
            unit //= 2
        has_bias = members[0][2] is not None
        if any((b is not None) != has_bias for (_, _, b) in members):
            raise _lib.SdnqHipError("grouped matmul: either every layer has a bias or none has")
        self.k = int(members[0][0].shape[1])
        self.keep = []  # the tensors the table points into
        rows = []
        n_start = 0
        for (w, ws, bias) in members:
            _require_cuda(w, ws, bias)
            n = int(w.shape[0])
            if w.shape[1] != self.k or not w.is_contiguous() or w.element_size() != 1:
                raise _lib.SdnqHipError("grouped matmul: weights must be contiguous [N, K] 1-byte operands of one K")
            ws = ws.reshape(-1)
            if ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() != n:
                raise _lib.SdnqHipError("grouped matmul: scales must be contiguous float32 [N]")
            if bias is not None:
                bias = bias.contiguous()
                if bias.dtype != members[0][2].dtype:
                    raise _lib.SdnqHipError("grouped matmul: one bias dtype per group")
            self.keep.append((w, ws, bias))
            for loc in range(0, n, unit):
                rows.append((w.data_ptr() + loc * self.k, ws.data_ptr() + 4 * loc,
                             0 if bias is None else bias.data_ptr() + loc * bias.element_size(), n_start, n, loc))
            n_start += n
        table = np.array(rows, dtype=np.dtype(_lib.SdnqGemmUnit))  # b, sb, bias, n_start, n_seg, n_loc: the struct's own layout
        self.device = members[0][0].device
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(self.device)
        self.n_units, self.unit_n, self.n_total = len(rows), unit, n_start
        self.widths = ns
        self.bias_dtype = float_code(members[0][2].dtype) if has_bias else -1
        self.mm_torch = members[0][0].dtype


def scaled_mm_grouped(mm: int, a: torch.Tensor, sa: torch.Tensor, group: GemmGroup, out_dtype: torch.dtype):
    """One launch for every layer of `group` on the shared quantized activation a [M, K]; returns one contiguous [M, N_i] tensor
    per layer (views of ONE allocation), each bit-identical to scaled_mm on that layer alone."""
    _require_cuda(a, sa)
    m, k = a.shape
    if k != group.k:
        raise _lib.SdnqHipError(f"grouped matmul: activation has K={k}, the group K={group.k}")
    out = torch.empty((m * group.n_total,), device=a.device, dtype=out_dtype)
    check(_lib.load().sdnq_hip_scaled_mm_grouped(mm, a.data_ptr(), sa.data_ptr(), group.table.data_ptr(), group.n_units, group.unit_n,
                                                 group.bias_dtype, out.data_ptr(), float_code(out_dtype), m, k, _stream(a)),
          "scaled_mm_grouped")
    outs, start = [], 0
    for n in group.widths:
        outs.append(out[m * start:m * (start + n)].view(m, n))
        start += n
    return outs


def linear_float_multi(x2d: torch.Tensor, wd: torch.Tensor, bias, n_outs: int):
    """F.linear over the stacked dequantized weights of `n_outs` layers, one contiguous output per layer (M > 32)."""
    _require_cuda(x2d, wd)
    m, k = x2d.shape
    n = wd.shape[0]
    seg = n // n_outs
    outs = [torch.empty((m, seg), device=x2d.device, dtype=x2d.dtype) for _ in range(n_outs)]
    ptrs = (ctypes.c_void_p * n_outs)(*[o.data_ptr() for o in outs])
    check(_lib.load().sdnq_hip_linear_float_multi(x2d.data_ptr(), wd.data_ptr(), _ptr(bias), float_code(x2d.dtype), ptrs, n_outs, seg,
                                                  m, n, k, x2d.stride(0), _stream(x2d)), "linear_float_multi")
    return outs


def linear_w8a8(mm: int, x2d: torch.Tensor, b_phys: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype, hadamard_group: int = 0):
    """rowquant + scaled_mm through ONE binding call (two launches) -> (out [M,N], xq [M,K], xs [M,1])."""
    m, k = x2d.shape
    n = b_phys.shape[0]
    dev = x2d.device
    xq = torch.empty((m, k), device=dev, dtype=_MM_TORCH[mm])
    xs = torch.empty((m, 1), device=dev, dtype=torch.float32)
    out = torch.empty((m, n), device=dev, dtype=out_dtype)
    bias_dt = 0
    if bias is not None:
        bias_dt = float_code(bias.dtype)
    check(_lib.load().sdnq_hip_linear_w8a8(mm, x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), hadamard_group, xq.data_ptr(),
                                           xs.data_ptr(), b_phys.data_ptr(), sb.data_ptr(), _ptr(bias), bias_dt, out.data_ptr(),
                                           float_code(out_dtype), n, _stream(x2d)), "linear_w8a8")
    return out, xq, xs


def linear_w8a8_ws(mm: int, x2d: torch.Tensor, b_phys: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype, hadamard_group: int = 0):
    """linear_w8a8 with the quantized activation in the stream's persistent scratch buffer (not returned, not kept): ONE allocation
    per call instead of three.  Same-stream launches are ordered, so the next layer overwriting the buffer is safe; a buffer replaced
    by a larger one stays valid for the work already queued (the caching allocator does not hand a freed block to another stream).
    While the stream is being captured into a graph the scratch is a fresh tensor of the graph's pool instead (the shared buffer
    may be replaced later)."""
    m, k = x2d.shape
    n = b_phys.shape[0]
    stream = _stream(x2d)
    xq_bytes = (m * k + 255) & ~255
    if torch.cuda.is_current_stream_capturing():
        scratch = torch.empty((xq_bytes + 4 * m + 512 + 255,), device=x2d.device, dtype=torch.uint8)
    else:
        scratch = _workspace(x2d.device, stream, xq_bytes + 4 * m + 512)  # the per-stream scratch buffer (below)
    base = (scratch.data_ptr() + 255) & ~255
    out = torch.empty((m, n), device=x2d.device, dtype=out_dtype)
    check(_lib.load().sdnq_hip_linear_w8a8(mm, x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), hadamard_group, base,
                                           base + xq_bytes, b_phys.data_ptr(), sb.data_ptr(), _ptr(bias), 0 if bias is None else float_code(bias.dtype),
                                           out.data_ptr(), float_code(out_dtype), n, stream), "linear_w8a8")
    return out


def linear_w8a8_fused_supported(mm: int, x2d: torch.Tensor, n: int, out_dtype: torch.dtype) -> bool:
    """True where the ONE-launch w8a8 Linear (sdnq_hip_linear_w8a8_fused: the GEMM row-quantizes its own activation rows in LDS) is
    built and expected to win; the answer per (dtype, M, N, K) is memoized."""
    if x2d.dtype not in (torch.bfloat16, torch.float16) or out_dtype != x2d.dtype or not x2d.is_cuda or x2d.stride(0) * 128 >= (1 << 31):
        return False  # (a tile's 64 rows are addressed with 32-bit byte offsets)
    key = (mm, x2d.dtype, x2d.shape[0], n, x2d.shape[1], x2d.device.index)  # (per device: the answer depends on its CU count)
    r = _fused_ok.get(key)
    if r is None:
        with torch.cuda.device(x2d.device):
            r = bool(_lib.load().sdnq_hip_linear_w8a8_fused_supported(mm, float_code(x2d.dtype), float_code(out_dtype), x2d.shape[0], n, x2d.shape[1]))
        _fused_ok[key] = r
    return r


_fused_ok = {}
fused_calls = [0]  # how many Linear calls took the one-launch route through THIS module (fused_call_count() adds the fast path's)


def fused_call_count() -> int:
    """Linear calls that took the one-launch route since reset_fused_calls() (bench.py reports it per step)."""
    fp = _lib.fastpath()
    return fused_calls[0] + (fp.fused_calls() if fp is not None else 0)


def reset_fused_calls():
    fused_calls[0] = 0
    fp = _lib.fastpath()
    if fp is not None:
        fp.reset_counters()


def aq_slab_bytes(n: int, k: int) -> int:
    """Bytes of the fragment-ordered copy of an [n][k] int8 weight (sdnq_hip_aq_slab_bytes; 0 where none is defined)."""
    return int(_lib.load().sdnq_hip_aq_slab_bytes(n, k))


_slab_wanted = {}


def aq_slab_wanted(mm: int, m: int, n: int, k: int, device) -> bool:
    """True where the one-launch Linear on (m, n, k) would read the slab copy of its weight (sdnq_hip_aq_slab_wanted; memoized per device)."""
    key = (mm, m, n, k, device.index)
    r = _slab_wanted.get(key)
    if r is None:
        with torch.cuda.device(device):
            r = _slab_wanted[key] = bool(_lib.load().sdnq_hip_aq_slab_wanted(mm, m, n, k))
    return r


def aq_slab_pack(b_phys: torch.Tensor) -> torch.Tensor:
    """The fragment-ordered copy of an int8 weight [N][K] (row stride >= K) for the one-launch Linear's 32 x 256 tile: a new int8 tensor
    of aq_slab_bytes(N, K) bytes, written on the current stream (sdnq_hip_aq_slab_pack)."""
    _require_cuda(b_phys)
    n, k = b_phys.shape
    nbytes = aq_slab_bytes(n, k)
    if nbytes == 0 or b_phys.stride(1) != 1 or b_phys.element_size() != 1:
        raise _lib.SdnqHipError(f"aq_slab_pack: no slab copy for a weight of shape {tuple(b_phys.shape)}, strides {b_phys.stride()}, {b_phys.dtype}")
    out = torch.empty(nbytes, device=b_phys.device, dtype=torch.int8)
    check(_lib.load().sdnq_hip_aq_slab_pack(b_phys.data_ptr(), n, k, b_phys.stride(0), out.data_ptr(), _stream(b_phys)), "aq_slab_pack")
    return out


def linear_w8a8_fused(mm: int, x2d: torch.Tensor, b_phys: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype, slab=None) -> torch.Tensor:
    """The plain w8a8 Linear as one launch (no quantized copy of the activation is produced); bit-identical to linear_w8a8.
    `slab`: aq_slab_pack(b_phys), or None -- where the launch runs the 32 x 256 tile its waves read their weights from it."""
    _require_cuda(x2d, b_phys, sb, bias)
    m, k = x2d.shape
    n = b_phys.shape[0]
    out = torch.empty((m, n), device=x2d.device, dtype=out_dtype)
    if bias is not None:
        bias = bias.contiguous()
    fused_calls[0] += 1
    if slab is not None:
        check(_lib.load().sdnq_hip_linear_w8a8_fused_slab(mm, x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), b_phys.data_ptr(), sb.data_ptr(),
                                                          _ptr(bias), 0 if bias is None else float_code(bias.dtype), out.data_ptr(), float_code(out_dtype),
                                                          n, slab.data_ptr(), _stream(x2d)), "linear_w8a8_fused_slab")
        return out
    check(_lib.load().sdnq_hip_linear_w8a8_fused(mm, x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), b_phys.data_ptr(), sb.data_ptr(),
                                                 _ptr(bias), 0 if bias is None else float_code(bias.dtype), out.data_ptr(), float_code(out_dtype),
                                                 n, _stream(x2d)), "linear_w8a8_fused")
    return out


_fused_grouped_ok = {}


def linear_w8a8_fused_grouped_supported(mm: int, x2d: torch.Tensor, n_member: int, n_members: int, out_dtype: torch.dtype) -> bool:
    """True where the grouped one-launch Linear (sdnq_hip_linear_w8a8_fused_grouped) takes n_members layers of n_member channels on x2d;
    memoized per (dtype, M, widths, K, device) like linear_w8a8_fused_supported."""
    if x2d.dtype not in (torch.bfloat16, torch.float16) or out_dtype != x2d.dtype or not x2d.is_cuda or x2d.stride(0) * 128 >= (1 << 31):
        return False
    key = (mm, x2d.dtype, x2d.shape[0], n_member, n_members, x2d.shape[1], x2d.device.index)
    r = _fused_grouped_ok.get(key)
    if r is None:
        with torch.cuda.device(x2d.device):
            r = _fused_grouped_ok[key] = bool(_lib.load().sdnq_hip_linear_w8a8_fused_grouped_supported(
                mm, float_code(x2d.dtype), float_code(out_dtype), x2d.shape[0], n_member, n_members, x2d.shape[1]))
    return r


def linear_w8a8_fused_grouped(mm: int, x2d: torch.Tensor, members, out_dtype: torch.dtype):
    """One launch for layers that read the same activation x2d [M, K], no row-quantization launch in front of it.  `members`:
    [(slab, ws [N] f32, bias [N] | None)] with slab = aq_slab_pack of the layer's [N, K] int8 operand, one N for all.  Returns one
    contiguous [M, N] tensor per layer (views of ONE allocation, as scaled_mm_grouped), each bit-identical to linear_w8a8_fused on
    that layer alone."""
    m, k = x2d.shape
    g = len(members)
    n = int(members[0][1].numel())
    has_bias = members[0][2] is not None
    keep = []
    for (slab, ws, bias) in members:
        _require_cuda(x2d, slab, ws, bias)
        if ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() != n or slab.numel() != aq_slab_bytes(n, k) or not slab.is_contiguous():
            raise _lib.SdnqHipError("linear_w8a8_fused_grouped: every layer needs contiguous float32 scales [N] and the slab copy of an [N, K] operand, one N")
        if (bias is not None) != has_bias or (has_bias and (bias.numel() != n or bias.dtype != members[0][2].dtype)):
            raise _lib.SdnqHipError("linear_w8a8_fused_grouped: either every layer has a bias [N] of one dtype or none has")
        keep.append(None if bias is None else bias.contiguous())
    ptrs = ctypes.c_void_p * g
    slabs, sbs = ptrs(*[s.data_ptr() for (s, _, _) in members]), ptrs(*[w.data_ptr() for (_, w, _) in members])
    biases = ptrs(*[b.data_ptr() for b in keep]) if has_bias else None
    out = torch.empty((m * g * n,), device=x2d.device, dtype=out_dtype)
    fused_calls[0] += 1
    check(_lib.load().sdnq_hip_linear_w8a8_fused_grouped(mm, x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), slabs, sbs, biases,
                                                         float_code(keep[0].dtype) if has_bias else 0, g, n, out.data_ptr(), float_code(out_dtype),
                                                         _stream(x2d)), "linear_w8a8_fused_grouped")
    return [out[m * n * i:m * n * (i + 1)].view(m, n) for i in range(g)]


def scaled_mm_nchw(mm: int, a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype,
                   batch: int, pixels: int) -> torch.Tensor:
    """Conv flavour of scaled_mm: rows m = (b, pixel); returns the channel-major image [batch, N, pixels] (the reference's
    .view(B, H, W, C).permute(0, 3, 1, 2).contiguous(), conv_int8.py:81-88, fused into the epilogue)."""
    _require_cuda(a, b_phys, sa, sb, bias)
    m, k = a.shape
    n = b_phys.shape[0]
    assert m == batch * pixels
    out = torch.empty((batch, n, pixels), device=a.device, dtype=out_dtype)
    bias_dt = 0
    if bias is not None:
        bias = bias.contiguous()
        bias_dt = float_code(bias.dtype)
    check(_lib.load().sdnq_hip_scaled_mm_nchw(mm, a.data_ptr(), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias), bias_dt,
                                              out.data_ptr(), float_code(out_dtype), m, n, k, pixels, _stream(a)), "scaled_mm_nchw")
    return out


def scaled_mm_into(mm: int, a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, out: torch.Tensor,
                   chan0: int, pixels: int = 0) -> None:
    """scaled_mm on views (sdnq_hip_scaled_mm_strided): `a` is a column slice [M, K] of a wider row-major matrix, the N = b_phys.shape[0]
    output channels go to channels chan0 .. chan0 + N of `out` -- [M, C] row-major (pixels == 0) or the conv image [B, C, pixels].
    One group of a grouped conv (conv_int8.py:73-79)."""
    _require_cuda(a, b_phys, sa, sb, bias, out)
    m, k = a.shape
    n = b_phys.shape[0]
    assert a.stride(1) == 1 and b_phys.is_contiguous() and out.is_contiguous()
    c_total = out.shape[1]
    esz = out.element_size()
    dst = out.data_ptr() + (chan0 * pixels * esz if pixels else chan0 * esz)
    bias_dt = 0
    if bias is not None:
        bias = bias.contiguous()
        bias_dt = float_code(bias.dtype)
    check(_lib.load().sdnq_hip_scaled_mm_strided(mm, a.data_ptr(), a.stride(0), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias),
                                                 bias_dt, dst, c_total, float_code(out.dtype), m, n, k, pixels, _stream(a)), "scaled_mm_strided")


def scaled_mm_zp_into(mm: int, a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, rowsum, zp, a_zp, w_colsum_scaled,
                      zp_k: int, out: torch.Tensor, chan0: int) -> None:
    """scaled_mm with the zero-point / activation-zero-point epilogue terms on views (sdnq_hip_scaled_mm_lowrank_strided): one group of a
    grouped conv with unsigned weights or the uint8 matmul (conv_int8.py:65-79, conv_uint8.py:58-79).  `rowsum` / `a_zp` are per ROW
    of the whole unfolded input, `sb / bias / zp / w_colsum_scaled` this group's channels, `zp_k` the whole row's K; the N results go to
    columns chan0 .. chan0 + N of the row-major `out` [M, C]."""
    _require_cuda(a, b_phys, sa, sb, bias, rowsum, zp, a_zp, w_colsum_scaled, out)
    m, k = a.shape
    n = b_phys.shape[0]
    assert a.stride(1) == 1 and b_phys.is_contiguous() and out.is_contiguous() and out.dim() == 2
    bias_dt = 0
    if bias is not None:
        bias = bias.contiguous()
        bias_dt = float_code(bias.dtype)
    check(_lib.load().sdnq_hip_scaled_mm_lowrank_strided(mm, a.data_ptr(), a.stride(0), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias),
                                                         bias_dt, _ptr(rowsum), _ptr(zp), _ptr(a_zp), _ptr(w_colsum_scaled), int(zp_k),
                                                         out.data_ptr() + chan0 * out.element_size(), out.shape[1], float_code(out.dtype), m, n, k,
                                                         _stream(a)), "scaled_mm_lowrank_strided")


def linear_float_into(x2d: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, chan0: int) -> None:
    """linear_float on views (sdnq_hip_linear_float_strided): x2d a column slice [M, K], the N outputs go to columns chan0 .. chan0 + N of
    the row-major `out` [M, C]."""
    _require_cuda(x2d, w, bias, out)
    m, k = x2d.shape
    n = w.shape[0]
    assert w.is_contiguous() and x2d.stride(1) == 1 and w.dtype == x2d.dtype == out.dtype and out.is_contiguous()
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    check(_lib.load().sdnq_hip_linear_float_strided(x2d.data_ptr(), w.data_ptr(), _ptr(bias), float_code(x2d.dtype),
                                                    out.data_ptr() + chan0 * out.element_size(), m, n, k, x2d.stride(0), out.shape[1],
                                                    _stream(x2d)), "linear_float_strided")


def scaled_mm_lowrank(mm: int, a, b_phys, sa, sb, bias, t, svd_up_phys, rowsum, zp, out_dtype: torch.dtype, a_zp=None,
                      w_colsum_scaled=None):
    _require_cuda(a, b_phys)
    m, k = a.shape
    n = b_phys.shape[0]
    out = torch.empty((m, n), device=a.device, dtype=out_dtype)
    rank = 0 if t is None else t.shape[1]
    svd_dt = 0 if t is None else float_code(t.dtype)
    bias_dt = 0
    if bias is not None:
        if t is not None and bias.dtype != t.dtype:
            bias = bias.to(t.dtype)  # bias.to(dtype=svd_down.dtype), linear_int8.py:60
        bias = bias.contiguous()
        bias_dt = float_code(bias.dtype)
    check(_lib.load().sdnq_hip_scaled_mm_lowrank(mm, a.data_ptr(), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias),
                                                 bias_dt, _ptr(t), _ptr(svd_up_phys), svd_dt, rank, _ptr(rowsum), _ptr(zp),
                                                 _ptr(a_zp), _ptr(w_colsum_scaled), out.data_ptr(), float_code(out_dtype), m, n, k, _stream(a)), "scaled_mm_lowrank")
    return out


def dequant(qw: QuantWeight, out_dtype: torch.dtype, hadamard_group: int = 0, use_svd: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
    dev = qw.keep[0].device
    if out is None:
        out = torch.empty((qw.n, qw.k), device=dev, dtype=out_dtype)
    d = qw.desc
    if not use_svd and d.svd_up:
        d = SdnqWeight.from_buffer_copy(bytes(d))
        d.svd_up = None
        d.svd_down = None
        d.svd_rank = 0
    check(_lib.load().sdnq_hip_dequant(ctypes.byref(d), hadamard_group, out.data_ptr(), float_code(out_dtype),
                                       torch.cuda.current_stream(dev).cuda_stream), "dequant")
    return out


def dequant_t(qw: QuantWeight, out_dtype: torch.dtype, out: torch.Tensor | None = None) -> torch.Tensor:
    """sdnq_hip_dequant_t: the dequantized weight transposed, [K, N] contiguous -- ``dequant(qw, out_dtype, 0, use_svd=False).t()`` bit
    for bit, decoded from the stored codes in one launch.  No SVD factors, K % 16 == 0 and N % 8 == 0 (anything else raises)."""
    dev = qw.keep[0].device
    if out is None:
        out = torch.empty((qw.k, qw.n), device=dev, dtype=out_dtype)
    elif out.dtype != out_dtype or out.numel() != qw.n * qw.k or not out.is_contiguous():
        raise _lib.SdnqHipError(f"dequant_t: out must be {qw.k * qw.n} contiguous elements of {out_dtype}")
    check(_lib.load().sdnq_hip_dequant_t(ctypes.byref(qw.desc), out.data_ptr(), float_code(out_dtype), _stream(out)), "dequant_t")
    return out.view(qw.k, qw.n)


def transpose2d(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """sdnq_hip_transpose2d: x [R, C] (unit column stride, any row stride) -> [C, R] contiguous, the same bits."""
    _require_cuda(x, out)
    if x.ndim != 2 or x.stride(1) != 1:
        raise _lib.SdnqHipError(f"transpose2d takes a 2-D tensor with contiguous rows (got shape {tuple(x.shape)}, strides {x.stride()})")
    r, c = x.shape
    if out is None:
        out = torch.empty((c, r), device=x.device, dtype=x.dtype)
    elif out.dtype != x.dtype or out.numel() != r * c or not out.is_contiguous():
        raise _lib.SdnqHipError(f"transpose2d: out must be {r * c} contiguous elements of {x.dtype}")
    check(_lib.load().sdnq_hip_transpose2d(x.data_ptr(), float_code(x.dtype), r, c, x.stride(0), out.data_ptr(), _stream(x)), "transpose2d")
    return out.view(c, r)


def weight_t(qw: QuantWeight, out_dtype: torch.dtype, hadamard_group: int, scratch) -> torch.Tensor:
    """The weight a layer's forward multiplies by -- SVD product added, Hadamard rotation undone: the reference's weight.dequantize() --
    as the [K, N] operand of grad_input = linear_float(dY, weight_t), written into `scratch` and returned as a view of it.
    scratch: (first, second), 1-D tensors of `out_dtype` with at least N * K elements each; `second` may be None for a plain layer.
    A plain layer is decoded transposed in one launch (dequant_t); a layer with SVD factors or a rotation is dequantized into `second` by
    the kernels of its forward (dequant) and transposed into `first` (transpose2d): one more pass, the same bits."""
    first, second = scratch
    nk = qw.n * qw.k
    if not qw.desc.svd_up and not hadamard_group:
        return dequant_t(qw, out_dtype, out=first[:nk])
    if second is None:
        raise _lib.SdnqHipError("weight_t: a layer with SVD factors or a Hadamard rotation needs the second scratch buffer")
    wd = dequant(qw, out_dtype, hadamard_group, out=second[:nk].view(qw.n, qw.k))
    return transpose2d(wd, out=first[:nk])


def make_convt_weight(weights_dtype: str, weight: torch.Tensor, scale: torch.Tensor, zero_point, c_in: int, p_cols: int, kprod: int) -> QuantWeight:
    """The stored tensors of a transposed-conv layer ([C_in, C_out / groups, *kernel] codes or their packed form, element order
    [C_in][P]) as the descriptor sdnq_hip_dequant_convt reads: n = C_in, k = P = C_out / groups * prod(kernel), positions = prod(kernel).
    scale / zero_point: [1, C_out / groups, *kernel] (one per column, P values) or the square grouped layout
    [C_in, 1, num_groups, *kernel] (C_in * num_groups * prod(kernel) values) -- `QuantWeight.group_size` holds num_groups (1: per column)."""
    _require_cuda(weight, scale)
    storage, kind, bits, ebits, mbits, native = _storage_kind(weights_dtype)
    w_phys = weight if weight.is_contiguous() else weight.contiguous()
    if w_phys.dtype in (torch.int64, torch.bool):
        w_phys = w_phys.to(torch.uint8)
    scale_dtype = scale.dtype
    if scale_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise _lib.SdnqHipError(f"scale must be float32, bfloat16 or float16, got {scale_dtype}")
    if scale_dtype != torch.float32 and bits > 8:
        raise _lib.SdnqHipError("16-bit scales with formats wider than 8 bits are not built (the codes are not exact in the scale dtype)")
    if zero_point is not None and zero_point.dtype != scale_dtype:
        raise _lib.SdnqHipError("scale and zero_point must share one dtype (loader.py:277-280 casts both)")
    sc = scale.to(torch.float32).contiguous().view(-1)
    if sc.numel() == p_cols and (scale.ndim < 1 or scale.shape[0] == 1):
        num_groups = 1
    elif sc.numel() % (c_in * kprod) == 0 and scale.shape[0] == c_in:
        num_groups = sc.numel() // (c_in * kprod)
    else:
        raise _lib.SdnqHipError(f"scale of shape {tuple(scale.shape)} is neither [1, P] nor [C_in, 1, groups, *kernel] for C_in = {c_in}, P = {p_cols}")
    zp = None
    if zero_point is not None:
        zp = zero_point.to(torch.float32).contiguous().view(-1)
        if zp.numel() != sc.numel():
            raise _lib.SdnqHipError("zero_point size mismatch")
    d = SdnqWeight(weight=_ptr(w_phys), scale=_ptr(sc), zero_point=_ptr(zp), svd_up=None, svd_down=None, n=c_in, k=p_cols,
                   group_size=p_cols, svd_rank=0, svd_dtype=0, storage=storage, kind=kind, bits=bits, exponent=ebits, mantissa=mbits,
                   native_float=native, positions=kprod, scale_dtype=float_code(scale_dtype))
    return QuantWeight(desc=d, n=c_in, k=p_cols, group_size=num_groups, keep=(w_phys, sc, zp, None, None), scale_dtype=scale_dtype)


def dequant_convt(qw: QuantWeight, out_dtype: torch.dtype, groups: int = 1) -> torch.Tensor:
    """sdnq_hip_dequant_convt: the dequantized weight of a transposed conv as the float GEMM's operand [groups, P, C_in / groups]."""
    dev = qw.keep[0].device
    if qw.n % groups:
        raise _lib.SdnqHipError(f"groups={groups} does not divide the {qw.n} input channels")
    out = torch.empty((groups, qw.k, qw.n // groups), device=dev, dtype=out_dtype)
    check(_lib.load().sdnq_hip_dequant_convt(ctypes.byref(qw.desc), groups, qw.group_size, out.data_ptr(), float_code(out_dtype),
                                             _stream(out)), "dequant_convt")
    return out


def linear_float_f32_into(x2d: torch.Tensor, w: torch.Tensor, out: torch.Tensor, col0: int) -> None:
    """sdnq_hip_linear_float_f32out_strided: x2d (a column slice [M, K]) . w[N, K]^T, unrounded, into columns col0 .. col0 + N of the
    row-major float32 `out` [M, C]."""
    _require_cuda(x2d, w, out)
    m, k = x2d.shape
    n = w.shape[0]
    assert w.is_contiguous() and x2d.stride(1) == 1 and w.dtype == x2d.dtype and out.dtype == torch.float32 and out.is_contiguous()
    assert 0 <= col0 and col0 + n <= out.shape[1] and out.shape[0] == m and w.shape[1] == k
    check(_lib.load().sdnq_hip_linear_float_f32out_strided(x2d.data_ptr(), w.data_ptr(), float_code(x2d.dtype),
                                                           out.data_ptr() + col0 * 4, m, n, k, x2d.stride(0), out.shape[1],
                                                           _stream(x2d)), "linear_float_f32out_strided")


def col2im(cols: torch.Tensor, bias, out_dtype: torch.dtype, batch: int, channels: int, in_size, out_size, kernel, stride, padding,
           dilation) -> torch.Tensor:
    """sdnq_hip_col2im: the gather half of a transposed convolution.  cols float32 [batch * prod(in_size), >= channels * prod(kernel)];
    in_size / out_size / kernel / stride / padding / dilation: 1 to 3 entries each -> [batch, channels, *out_size] of out_dtype.
    Limits of the launch: batch * ceil(prod(out_size) / 16) < 2^31 and channels <= 16 * 65535 (SDNQ_ERR_SHAPE beyond)."""
    _require_cuda(cols, bias)
    nd = len(in_size)
    lead = 3 - nd

    def three(v, fill):
        return [fill] * lead + [int(e) for e in v]
    i3, o3, k3, s3, p3, d3 = three(in_size, 1), three(out_size, 1), three(kernel, 1), three(stride, 1), three(padding, 0), three(dilation, 1)
    if cols.dtype != torch.float32 or cols.ndim != 2 or cols.stride(1) != 1 or cols.shape[0] != batch * i3[0] * i3[1] * i3[2]:
        raise _lib.SdnqHipError("col2im expects float32 cols [batch * input positions, columns]")
    if bias is not None:
        bias = bias.to(out_dtype).contiguous()
        if bias.numel() != channels:
            raise _lib.SdnqHipError("col2im: bias must hold one value per output channel")
    out = torch.empty((batch, channels, *[int(e) for e in out_size]), device=cols.device, dtype=out_dtype)
    check(_lib.load().sdnq_hip_col2im(cols.data_ptr(), cols.stride(0), _ptr(bias), float_code(out_dtype), out.data_ptr(), batch, channels,
                                      *i3, *o3, *k3, *s3, *p3, *d3, _stream(cols)), "col2im")
    return out


def dequant_loss_sum(qw: QuantWeight, ref: torch.Tensor, hadamard_group: int = 0) -> torch.Tensor:
    """sum((dequant(qw, float32, hadamard_group) - ref) ** 2) over [N][K] as a device fp64 scalar, in one fused pass that never writes
    the dequantized weight (sdnq_hip_dequant_loss; each term (d * d) in fp32, the sum in fp64, bitwise the same on every call).
    ref: the original float weight, [N, K] (or any shape whose leading dim is N and the rest flattens to K), fp32 / bf16 / f16, rows
    of unit stride.  Runs on torch's current stream; nothing is synchronised."""
    _require_cuda(ref)
    dev = qw.keep[0].device
    if ref.device != dev:
        raise _lib.SdnqHipError(f"dequant_loss: ref on {ref.device}, weight on {dev}")
    r = ref.reshape(qw.n, -1) if ref.dim() != 2 else ref
    if tuple(r.shape) != (qw.n, qw.k):
        raise _lib.SdnqHipError(f"dequant_loss: ref shape {tuple(ref.shape)} is not [N, K] = ({qw.n}, {qw.k})")
    if r.stride(1) != 1 or r.data_ptr() % 16 or (r.stride(0) * r.element_size()) % 16:
        r = r.contiguous()
    lib = _lib.load()
    nbytes = int(lib.sdnq_hip_dequant_loss_workspace_bytes(qw.n, qw.k))
    check(nbytes if nbytes < 0 else 0, "dequant_loss_workspace_bytes")
    ws = torch.empty((nbytes // 8 + 1,), device=dev, dtype=torch.float64)
    out = ws[-1:]
    check(lib.sdnq_hip_dequant_loss(ctypes.byref(qw.desc), hadamard_group, r.data_ptr(), float_code(r.dtype), r.stride(0), out.data_ptr(),
                                    ws.data_ptr(), nbytes, _stream(r)), "dequant_loss")
    return out.view(())


def dequant_loss(qw: QuantWeight, ref: torch.Tensor, hadamard_group: int = 0) -> float:
    """`dequant_loss_sum` read back to the host once (one synchronisation): the fp64 sum of squared reconstruction errors."""
    return float(dequant_loss_sum(qw, ref, hadamard_group).item())


def embedding(qw: QuantWeight, ids: torch.Tensor, out_dtype: torch.dtype, hadamard_group: int = 0, embed_scale: float | None = None) -> torch.Tensor:
    """quantized_embedding (layers/embedding/forward.py:14-68) in one launch: out = ids.shape + [D] rows of the dequantized table
    (SVD added, Hadamard rotation, then * embed_scale).  ids: int32 / int64 of any shape on the table's device; an id outside
    [0, V) gives a row of NaN (the kernel clamps its read index, nothing is checked on the host)."""
    _require_cuda(ids)
    if ids.dtype not in (torch.int32, torch.int64):
        raise _lib.SdnqHipError(f"embedding ids must be int32 or int64, got {ids.dtype}")
    dev = qw.keep[0].device
    if ids.device != dev:
        raise _lib.SdnqHipError(f"embedding ids on {ids.device}, table on {dev}")
    flat = ids if ids.is_contiguous() else ids.contiguous()
    out = torch.empty((*ids.shape, qw.k), device=dev, dtype=out_dtype)
    check(_lib.load().sdnq_hip_embedding(ctypes.addressof(qw.desc), hadamard_group, flat.data_ptr(),
                                         _lib.IDS_I64 if ids.dtype == torch.int64 else _lib.IDS_I32, flat.numel(),
                                         0 if embed_scale is None else 1, 0.0 if embed_scale is None else float(embed_scale),
                                         out.data_ptr(), float_code(out_dtype), _stream(flat)), "embedding")
    return out


def requant(qw: QuantWeight, mm: int, ws: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """re_quantize_int_mm / re_quantize_fp_mm (dequantizer.py:166-174, 204-239): (wq [N, K] int8 | fp8, ws [N] f32).  `ws`: the row
    scales of an earlier call on the same weights (sdnq_hip_requant_ws: the pass that derives them is skipped where the kernel can).
    `out`: caller-owned byte buffer of at least N * K bytes (16-byte aligned) the operand is written into (the per-call mode's
    double-buffered scratch); the returned wq is a view of it.  Runs on torch's CURRENT stream."""
    dev = qw.keep[0].device
    if out is not None:
        assert out.is_cuda and out.element_size() == 1 and out.numel() >= qw.n * qw.k and out.data_ptr() % 16 == 0
        wq = out[: qw.n * qw.k].view(_MM_TORCH[mm]).view(qw.n, qw.k)
    else:
        wq = torch.empty((qw.n, qw.k), device=dev, dtype=_MM_TORCH[mm])
    known = ws is not None
    if not known:
        ws = torch.empty((qw.n,), device=dev, dtype=torch.float32)
    check(_lib.load().sdnq_hip_requant_ws(ctypes.byref(qw.desc), mm, wq.data_ptr(), ws.data_ptr(), 1 if known else 0,
                                          torch.cuda.current_stream(dev).cuda_stream), "requant")
    return wq, ws


def lut4_build(qw: QuantWeight, mm: int, ws: torch.Tensor | None = None):
    """The re-quantization tables of a 4-bit weight (sdnq_hip_lut4_build): (lut uint8 [N, K / 64, 16], ws [N] f32) -- entry c of a table is
    the byte `requant` writes for code c in that 64-column block of that row.  Built once per layer; the operand of scaled_mm_w4."""
    dev = qw.keep[0].device
    lut = torch.empty((qw.n, qw.k // 64, 16), device=dev, dtype=torch.uint8)
    known = ws is not None
    if not known:
        ws = torch.empty((qw.n,), device=dev, dtype=torch.float32)
    check(_lib.load().sdnq_hip_lut4_build(ctypes.byref(qw.desc), mm, ws.data_ptr(), 1 if known else 0, lut.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), "lut4_build")
    return lut, ws


def scaled_mm_w4_supported(mm: int, m: int, n: int, k: int, out_dtype: torch.dtype) -> bool:
    return out_dtype in (torch.bfloat16, torch.float16) and bool(_lib.load().sdnq_hip_scaled_mm_w4_supported(mm, float_code(out_dtype), m, n, k))


def scaled_mm_w4(a: torch.Tensor, codes: torch.Tensor, lut: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype):
    """The quantized matmul on the STORED 4-bit codes (sdnq_hip_scaled_mm_w4): bit for bit scaled_mm(a, requant(weight), ...).
    a [M, K] int8 (row stride >= K), codes: the packed weight tensor (N * K / 2 bytes), lut: lut4_build's tables."""
    _require_cuda(a, codes, lut, sa, sb, bias)
    m, k = a.shape
    n = lut.shape[0]
    if a.stride(-1) != 1 or codes.numel() * codes.element_size() != n * k // 2 or not codes.is_contiguous() or tuple(lut.shape) != (n, k // 64, 16):
        raise _lib.SdnqHipError("scaled_mm_w4: a [M, K] int8 (unit inner stride), contiguous packed codes of N * K / 2 bytes, lut [N, K / 64, 16]")
    out = torch.empty((m, n), device=a.device, dtype=out_dtype)
    check(_lib.load().sdnq_hip_scaled_mm_w4(a.data_ptr(), codes.data_ptr(), lut.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias),
                                            0 if bias is None else float_code(bias.dtype), out.data_ptr(), float_code(out_dtype), m, n, k,
                                            a.stride(0), _stream(a)), "scaled_mm_w4")
    return out


def rowquant_f16(x2d: torch.Tensor):
    """quantize_fp_mm_input(..., matmul_dtype="float16") (linear_fp8.py:15-22, quant_utils.py:290-299): (xq float16 [M, K], xs f32 [M])."""
    _require_cuda(x2d)
    m, k = x2d.shape
    if x2d.stride(-1) != 1:
        raise _lib.SdnqHipError("rowquant_f16: unit inner stride")
    xq = torch.empty((m, k), device=x2d.device, dtype=torch.float16)
    xs = torch.empty((m,), device=x2d.device, dtype=torch.float32)
    check(_lib.load().sdnq_hip_rowquant_f16(x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), xq.data_ptr(), xs.data_ptr(), _stream(x2d)), "rowquant_f16")
    return xq, xs


def unpack_mm_f16(qw: QuantWeight) -> torch.Tensor:
    """Stored float codes -> float16 matmul operand [N, K] (linear_fp16.py:27-31)."""
    dev = qw.keep[0].device
    wq = torch.empty((qw.n, qw.k), device=dev, dtype=torch.float16)
    check(_lib.load().sdnq_hip_unpack_mm(ctypes.byref(qw.desc), _lib.MM_F16, wq.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "unpack_mm_f16")
    return wq


def scaled_mm_f16(a: torch.Tensor, b_phys: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, bias, out_dtype: torch.dtype) -> torch.Tensor:
    """fp_scaled_mm_func on float16 operands (kernel_wrappers.py:207-211): a [M, K] f16, b_phys [N, K] f16 -> [M, N]; bias None, [N] or the
    [M, N] low-rank term of a layer with SVD factors (linear_fp16.py:38-43)."""
    _require_cuda(a, b_phys, sa, sb, bias)
    m, k = a.shape
    n = b_phys.shape[0]
    if a.dtype != torch.float16 or b_phys.dtype != torch.float16 or not a.is_contiguous() or not b_phys.is_contiguous() or b_phys.shape[1] != k:
        raise _lib.SdnqHipError("scaled_mm_f16: contiguous float16 operands a [M, K], b [N, K]")
    nd, ldb = 0, 0
    if bias is not None:
        bias = bias.contiguous()
        nd = bias.dim()
        if nd == 2:
            if tuple(bias.shape) != (m, n):
                raise _lib.SdnqHipError("scaled_mm_f16: a 2-D bias must be [M, N]")
            ldb = bias.stride(0)
        elif nd != 1 or bias.numel() != n:
            raise _lib.SdnqHipError("scaled_mm_f16: bias must be [N] or [M, N]")
    out = torch.empty((m, n), device=a.device, dtype=out_dtype)
    check(_lib.load().sdnq_hip_scaled_mm_f16(a.data_ptr(), b_phys.data_ptr(), sa.data_ptr(), sb.data_ptr(), _ptr(bias), 0 if bias is None else float_code(bias.dtype),
                                             nd, ldb, out.data_ptr(), float_code(out_dtype), m, n, k, _stream(a)), "scaled_mm_f16")
    return out


def requant_asym(qw: QuantWeight):
    """re_quantize_uint_mm (dequantizer.py:178-187): (wq int8 [N,K], ws [N], zero_point [N])."""
    dev = qw.keep[0].device
    wq = torch.empty((qw.n, qw.k), device=dev, dtype=torch.int8)
    ws = torch.empty((qw.n,), device=dev, dtype=torch.float32)
    wzp = torch.empty((qw.n,), device=dev, dtype=torch.float32)
    check(_lib.load().sdnq_hip_requant_asym(ctypes.byref(qw.desc), wq.data_ptr(), ws.data_ptr(), wzp.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "requant_asym")
    return wq, ws, wzp


def unpack_mm(qw: QuantWeight, mm: int) -> torch.Tensor:
    """Stored codes -> matmul operand [N,K] without re-quantization (linear_int8.py:38-50, linear_fp8.py:36-38)."""
    dev = qw.keep[0].device
    wq = torch.empty((qw.n, qw.k), device=dev, dtype=_MM_TORCH[mm])
    check(_lib.load().sdnq_hip_unpack_mm(ctypes.byref(qw.desc), mm, wq.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
          "unpack_mm")
    return wq


def hadamard(x: torch.Tensor, group: int) -> torch.Tensor:
    _require_cuda(x)
    shape = x.shape
    x2 = x.reshape(-1, shape[-1])
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], x2.shape[1]), device=x.device, dtype=x.dtype)
    check(_lib.load().sdnq_hip_hadamard(x2.data_ptr(), float_code(x.dtype), x2.shape[0], x2.shape[1], x2.stride(0), group,
                                        y.data_ptr(), y.stride(0), _stream(x)), "hadamard")
    return y.view(shape)


def linear_float(x2d: torch.Tensor, w: torch.Tensor, bias) -> torch.Tensor:
    """x2d [M,K] @ w[N,K]^T + bias, all in one float dtype, fp32 accumulate."""
    _require_cuda(x2d, w, bias)
    m, k = x2d.shape
    n = w.shape[0]
    assert w.is_contiguous() and x2d.stride(1) == 1 and w.dtype == x2d.dtype
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    out = torch.empty((m, n), device=x2d.device, dtype=x2d.dtype)
    check(_lib.load().sdnq_hip_linear_float(x2d.data_ptr(), w.data_ptr(), _ptr(bias), float_code(x2d.dtype), out.data_ptr(),
                                            m, n, k, x2d.stride(0), _stream(x2d)), "linear_float")
    return out


def linear_w8a16(x2d: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, zero_point, bias) -> torch.Tensor:
    """Fused dequantize + float GEMM for row-wise 8-bit weights (sdnq_hip_linear_w8a16): x2d [M, K] bf16 / f16, w [N, K] int8 /
    uint8 physical, scale [N] f32, zero_point [N] f32 | None -> [M, N] of x2d's dtype."""
    _require_cuda(x2d, w, scale, zero_point, bias)
    m, k = x2d.shape
    n = w.shape[0]
    assert w.is_contiguous() and w.element_size() == 1 and x2d.stride(1) == 1 and scale.numel() == n
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    out = torch.empty((m, n), device=x2d.device, dtype=x2d.dtype)
    check(_lib.load().sdnq_hip_linear_w8a16(x2d.data_ptr(), float_code(x2d.dtype), w.data_ptr(), scale.data_ptr(), _ptr(zero_point), _ptr(bias),
                                            out.data_ptr(), m, n, k, x2d.stride(0), _stream(x2d)), "linear_w8a16")
    return out


def linear_w8a16_grouped(x2d: torch.Tensor, group: GemmGroup):
    """linear_w8a16 for every (signed int8, row-wise) layer of `group` in one launch; one contiguous [M, N_i] tensor per layer."""
    _require_cuda(x2d)
    m, k = x2d.shape
    if k != group.k or group.mm_torch != torch.int8:
        raise _lib.SdnqHipError("grouped fused dequantize GEMM: int8 weights of the activation's K")
    if group.bias_dtype >= 0 and group.bias_dtype != float_code(x2d.dtype):
        raise _lib.SdnqHipError("grouped fused dequantize GEMM: bias must have the activation dtype")
    out = torch.empty((m * group.n_total,), device=x2d.device, dtype=x2d.dtype)
    check(_lib.load().sdnq_hip_linear_w8a16_grouped(x2d.data_ptr(), float_code(x2d.dtype), group.table.data_ptr(), group.n_units, group.unit_n,
                                                    1 if group.bias_dtype >= 0 else 0, out.data_ptr(), m, k, x2d.stride(0), _stream(x2d)),
          "linear_w8a16_grouped")
    outs, start = [], 0
    for n in group.widths:
        outs.append(out[m * start:m * (start + n)].view(m, n))
        start += n
    return outs


def linear_skinny(qw: QuantWeight, x2d: torch.Tensor, bias, hadamard_group: int = 0) -> torch.Tensor:
    """Fused dequant (+ Hadamard un-rotation of the weight in registers) + float linear for M < 32 rows: streams the
    quantized weight once (no SVD)."""
    _require_cuda(x2d, bias)
    m, k = x2d.shape
    assert k == qw.k and x2d.stride(1) == 1
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    out = torch.empty((m, qw.n), device=x2d.device, dtype=x2d.dtype)
    check(_lib.load().sdnq_hip_linear_skinny(ctypes.byref(qw.desc), hadamard_group, x2d.data_ptr(), _ptr(bias), float_code(x2d.dtype), out.data_ptr(), m,
                                             x2d.stride(0), _stream(x2d)), "linear_skinny")
    return out


def linear_skinny_svd(qw: QuantWeight, svd_down_t: torch.Tensor, x2d: torch.Tensor, bias) -> torch.Tensor:
    """Few-row linear on an int8 row-wise weight with SVD factors; svd_down_t is [K, R] contiguous."""
    _require_cuda(x2d, bias, svd_down_t)
    m, k = x2d.shape
    assert k == qw.k and x2d.stride(1) == 1 and svd_down_t.is_contiguous()
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    out = torch.empty((m, qw.n), device=x2d.device, dtype=x2d.dtype)
    check(_lib.load().sdnq_hip_linear_skinny_svd(ctypes.byref(qw.desc), svd_down_t.data_ptr(), x2d.data_ptr(), _ptr(bias),
                                                 float_code(x2d.dtype), out.data_ptr(), m, x2d.stride(0), _stream(x2d)), "linear_skinny_svd")
    return out


def lowrank_down(x2d: torch.Tensor, svd_down_phys: torch.Tensor) -> torch.Tensor:
    """t[M,R] = cast(x2d @ svd_down_phys^T); svd_down_phys is physical [R,K]."""
    m, k = x2d.shape
    r = svd_down_phys.shape[0]
    t = torch.empty((m, r), device=x2d.device, dtype=svd_down_phys.dtype)
    check(_lib.load().sdnq_hip_lowrank_down(x2d.data_ptr(), float_code(x2d.dtype), m, k, x2d.stride(0), svd_down_phys.data_ptr(),
                                            float_code(svd_down_phys.dtype), r, t.data_ptr(), _stream(x2d)), "lowrank_down")
    return t


def _ld(t: torch.Tensor) -> int:
    """The row stride the library is given: the tensor's, or the row length for a single row (torch leaves the stride of a size-1 axis
    arbitrary, and nothing steps over it)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _rank_check(what: str, rank: int) -> None:
    if rank % 8 or not 8 <= rank <= 256:
        raise _lib.SdnqHipError(f"{what}: rank % 8 == 0 and 8 <= rank <= 256 (got rank = {rank})")


def _lowrank_check(what: str, rank: int, **tensors) -> None:
    """The checks the two adapter entry points share: device tensors of ONE 16-bit dtype, 8 <= rank <= 256 a multiple of 8, 2-D operands
    with contiguous, 16-byte aligned rows -- each failure names what is wrong.  (The device check comes last, in the callers: what a call
    gets wrong about shapes and dtypes does not depend on where its tensors live.)"""
    dt = next(iter(tensors.values())).dtype
    if dt not in (torch.bfloat16, torch.float16):
        raise _lib.SdnqHipError(f"{what}: built for bfloat16 / float16 operands (got {dt})")
    _rank_check(what, rank)
    for name, t in tensors.items():
        if t.dtype != dt:
            raise _lib.SdnqHipError(f"{what}: {name} must have the dtype of the other operands (got {t.dtype}, {dt})")
        if t.ndim != 2 or t.stride(1) != 1 or _ld(t) < t.shape[1]:
            raise _lib.SdnqHipError(f"{what}: {name} must be 2-D with contiguous rows (got shape {tuple(t.shape)}, strides {t.stride()})")
        if t.data_ptr() % 16 or (_ld(t) * 2) % 16:
            raise _lib.SdnqHipError(f"{what}: {name} is misaligned: its rows must start on 16 bytes (storage offset "
                                    f"{t.storage_offset()}, row stride {t.stride(0)} elements)")


def _lowrank_add(what: str, t: torch.Tensor, up: torch.Tensor, y: torch.Tensor, scale: float, drop=None, dora=None) -> torch.Tensor:
    """lowrank_add (drop and dora None), lowrank_add_dropout (drop = (threshold, seed, offset)) and lowrank_add_dora (dora = (c, bias | None)):
    the same checks under the caller's name.  drop and dora are exclusive, as in the library's launcher."""
    if t.ndim != 2 or up.ndim != 2 or y.ndim != 2:
        raise _lib.SdnqHipError(f"{what}: t, up and y must be 2-D (got {tuple(t.shape)}, {tuple(up.shape)}, {tuple(y.shape)})")
    (m, r), (n, r2) = t.shape, up.shape
    _lowrank_check(what, r, t=t, up=up, y=y)
    if r2 != r or tuple(y.shape) != (m, n):
        raise _lib.SdnqHipError(f"{what}: t [M, R], up [N, R], y [M, N] (got {tuple(t.shape)}, {tuple(up.shape)}, {tuple(y.shape)})")
    if n % 8:
        raise _lib.SdnqHipError(f"{what}: n % 8 == 0 (got n = {n}): y moves in 16-byte pieces")
    if not t.is_contiguous() or not up.is_contiguous():
        raise _lib.SdnqHipError(f"{what}: t and up must be contiguous")
    if drop is not None and dora is not None:
        raise _lib.SdnqHipError(f"{what}: the dropout mask and DoRA's epilogue are exclusive (no such kernel)")
    if drop is not None:
        drop = _dropout_args(what, *drop)
    if dora is not None:
        _dora_vectors(what, n, y.dtype, *dora)
    _require_cuda(t, up, y, *(dora or ()))
    if m == 0:
        return y
    head = (t.data_ptr(), up.data_ptr(), float_code(y.dtype), r, float(scale), y.data_ptr(), m, n, _ld(y))
    if dora is not None:
        check(_lib.load().sdnq_hip_lowrank_add_dora(*head, dora[0].data_ptr(), _ptr(dora[1]), _stream(y)), what)
    elif drop is None:
        check(_lib.load().sdnq_hip_lowrank_add(*head, _stream(y)), what)
    else:
        check(_lib.load().sdnq_hip_lowrank_add_dropout(*head, *drop, _stream(y)), what)
    return y


def lowrank_add(t: torch.Tensor, up: torch.Tensor, y: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """sdnq_hip_lowrank_add: y [M, N] += scale * t [M, R] @ up [N, R]^T IN PLACE on the matrix cores, every element rounded once:
    y = round(fma(scale, sum_r t up, y)).  bfloat16 / float16; y may be a column slice of a wider buffer (unit column stride, 16-byte
    aligned rows); t and up contiguous.  Returns y."""
    return _lowrank_add("lowrank_add", t, up, y, scale)


def lowrank_grad_workspace_bytes(m: int, p: int, rank: int) -> int:
    """sdnq_hip_lowrank_grad_workspace_bytes: 0 while the m rows fit one slab of the deterministic reduction."""
    nbytes = _lib.load().sdnq_hip_lowrank_grad_workspace_bytes(m, p, rank)
    if nbytes < 0:
        check(int(nbytes), "lowrank_grad_workspace_bytes")
    return int(nbytes)


def _grad_workspace(what: str, device: torch.device, stream: int, need: int, workspace):
    """The 16-byte aligned address of `need` bytes (None for 0) inside `workspace`, which the caller's _require_cuda has seen to be on the
    device, or for None inside the per-(device, stream) buffer of _workspace, which does not grow while its stream is being captured."""
    if not need:
        return None
    if workspace is None:
        have = _workspaces.get((device.index, stream))
        if (have is None or have.numel() < need + 16) and torch.cuda.is_current_stream_capturing():
            raise _lib.SdnqHipError(f"{what}: the module's workspace would have to grow inside a graph capture; pass workspace= or run "
                                    "one eager call on this stream first")
        workspace = _workspace(device, stream, need + 16)
    if workspace.dtype != torch.uint8 or workspace.numel() < need:
        raise _lib.SdnqHipError(f"{what}: workspace must be a uint8 device tensor of at least {need} bytes")
    wp = (workspace.data_ptr() + 15) & ~15
    if wp + need > workspace.data_ptr() + workspace.numel():
        raise _lib.SdnqHipError(f"{what}: workspace must hold {need} bytes behind its first 16-byte boundary")
    return wp


def _lowrank_grad(what: str, a: torch.Tensor, b: torch.Tensor, scale: float, out_t: bool, out_dtype, workspace, drop=None) -> torch.Tensor:
    """lowrank_grad (drop None) and lowrank_grad_dropout (drop = (threshold, seed, offset)): the same checks under the caller's name."""
    if a.ndim != 2 or b.ndim != 2:
        raise _lib.SdnqHipError(f"{what}: a and b must be 2-D (got {tuple(a.shape)}, {tuple(b.shape)})")
    (m, p), (m2, r) = a.shape, b.shape
    _lowrank_check(what, r, a=a, b=b)
    if m2 != m:
        raise _lib.SdnqHipError(f"{what}: a [M, P] and b [M, R] must have the same rows (got {tuple(a.shape)}, {tuple(b.shape)})")
    if p % 8:
        raise _lib.SdnqHipError(f"{what}: p % 8 == 0 (got p = {p}): a is read in 16-byte pieces")
    if not b.is_contiguous():
        raise _lib.SdnqHipError(f"{what}: b must be contiguous")
    if drop is not None:
        drop = _dropout_args(what, *drop)
    _require_cuda(a, b, workspace)
    out_dtype = a.dtype if out_dtype is None else out_dtype
    out = torch.empty((r, p) if out_t else (p, r), device=a.device, dtype=out_dtype)
    code = float_code(out_dtype)
    if m == 0:
        return out.zero_()
    need = lowrank_grad_workspace_bytes(m, p, r)
    wp = _grad_workspace(what, a.device, _stream(a), need, workspace)
    head = (a.data_ptr(), _ld(a), b.data_ptr(), float_code(a.dtype), m, p, r, float(scale), int(bool(out_t)), out.data_ptr(), code, wp, need)
    if drop is None:
        check(_lib.load().sdnq_hip_lowrank_grad(*head, _stream(a)), what)
    else:
        check(_lib.load().sdnq_hip_lowrank_grad_dropout(*head, *drop, _stream(a)), what)
    return out


def lowrank_grad(a: torch.Tensor, b: torch.Tensor, scale: float = 1.0, out_t: bool = False, out_dtype: torch.dtype | None = None,
                 workspace: torch.Tensor | None = None) -> torch.Tensor:
    """sdnq_hip_lowrank_grad: round(scale * a [M, P]^T @ b [M, R]) -> [P, R] (out_t: [R, P]) of `out_dtype` (default: the operands'),
    float32 sums on the matrix cores over slabs of rows added in a fixed order: the same bits on every call, no atomics.  a may be a
    column slice (unit column stride, 16-byte aligned rows), b contiguous; bfloat16 / float16.  workspace: a uint8 tensor of at least
    lowrank_grad_workspace_bytes(M, P, R) bytes, or None -- then the per-(device, stream) buffer of this module (_workspace: at least 1 MB,
    kept for the life of the process, NOT counted by training.scratch_bytes() nor freed by training.release_scratch(); sdnq_amd.lora passes
    the "partials" slot of sdnq_amd.scratch, which is) is used, and a call that would grow it while its stream is captured raises before any launch."""
    return _lowrank_grad("lowrank_grad", a, b, scale, out_t, out_dtype, workspace)


# ---- LoRA dropout: the three adapter kernels with the mask recomputed inside (include/sdnq_hip.h has the counter convention) -----------------
class _Dropout(typing.NamedTuple):
    """The dropout triple of one adapter call, in the order the library (and every ``lowrank_*_dropout`` here) takes it: splat it."""
    threshold: int
    seed: int
    offset: int


def _dropout_args(what: str, threshold: int, seed: int, offset: int) -> tuple:
    """(threshold, seed, offset) as the library takes them: an element is dropped iff its 16 random bits are < threshold."""
    threshold, seed, offset = int(threshold), int(seed), int(offset)
    if not 1 <= threshold <= 65535:
        raise _lib.SdnqHipError(f"{what}: 1 <= threshold <= 65535 (got threshold = {threshold}): the probability of a drop is threshold / 65536")
    if not (0 <= seed < 1 << 64 and 0 <= offset < 1 << 64):
        raise _lib.SdnqHipError(f"{what}: seed and offset are unsigned 64-bit integers (got seed = {seed}, offset = {offset})")
    return threshold, seed, offset


def lowrank_down_dropout(x2d: torch.Tensor, down: torch.Tensor, threshold: int, seed: int, offset: int) -> torch.Tensor:
    """sdnq_hip_lowrank_down_dropout: t [M, R] = round((mask * x2d) @ down [R, K]^T), the bits of ``lowrank_down`` on a pre-masked x2d
    without that tensor: element (i, j) of x2d is kept iff the 16 Philox bits of its LOGICAL index i K + j (key `seed`, `offset`, stream 5)
    are >= `threshold`.  Survivors are not rescaled (the caller's scale carries 1 / (1 - p)).  bfloat16 / float16, 16 | K; x2d may be
    row-strided (unit column stride, 16-byte aligned rows), down contiguous.  There is no float32 and no few-row path."""
    if x2d.ndim != 2 or down.ndim != 2:
        raise _lib.SdnqHipError(f"lowrank_down_dropout: x and down must be 2-D (got {tuple(x2d.shape)}, {tuple(down.shape)})")
    (m, k), (r, k2) = x2d.shape, down.shape
    _lowrank_check("lowrank_down_dropout", r, x=x2d, down=down)
    if k2 != k:
        raise _lib.SdnqHipError(f"lowrank_down_dropout: x [M, K] and down [R, K] (got {tuple(x2d.shape)}, {tuple(down.shape)})")
    if k % 16:
        raise _lib.SdnqHipError(f"lowrank_down_dropout: k % 16 == 0 (got k = {k}): the matrix-core kernel is the only path")
    if not down.is_contiguous():
        raise _lib.SdnqHipError("lowrank_down_dropout: down must be contiguous")
    threshold, seed, offset = _dropout_args("lowrank_down_dropout", threshold, seed, offset)
    _require_cuda(x2d, down)
    t = torch.empty((m, r), device=x2d.device, dtype=x2d.dtype)
    if m == 0:
        return t
    check(_lib.load().sdnq_hip_lowrank_down_dropout(x2d.data_ptr(), float_code(x2d.dtype), m, k, _ld(x2d), down.data_ptr(), r, t.data_ptr(),
                                                    threshold, seed, offset, _stream(x2d)), "lowrank_down_dropout")
    return t


def lowrank_add_dropout(t: torch.Tensor, up: torch.Tensor, y: torch.Tensor, scale: float, threshold: int, seed: int, offset: int) -> torch.Tensor:
    """sdnq_hip_lowrank_add_dropout: ``lowrank_add`` on the elements of y [M, N] that the mask keeps (logical index i N + j, as
    ``lowrank_down_dropout``); a dropped element keeps its bits.  IN PLACE; returns y."""
    return _lowrank_add("lowrank_add_dropout", t, up, y, scale, (threshold, seed, offset))


def lowrank_grad_dropout(a: torch.Tensor, b: torch.Tensor, scale: float, threshold: int, seed: int, offset: int, out_t: bool = False,
                         out_dtype: torch.dtype | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """sdnq_hip_lowrank_grad_dropout: round(scale * (mask * a [M, P])^T @ b [M, R]), the bits of ``lowrank_grad`` on a pre-masked a
    without that tensor (logical index i P + j, as ``lowrank_down_dropout``).  Everything else -- slabs, workspace, out_t, out_dtype -- as
    ``lowrank_grad``."""
    return _lowrank_grad("lowrank_grad_dropout", a, b, scale, out_t, out_dtype, workspace, (threshold, seed, offset))


# ---- DoRA on the Linear adapters (include/sdnq_hip.h has the arithmetic) ---------------------------------------------------------------------
def _dora_factors(what: str, n: int, k: int, up, down):
    """(rank, dtype code | None) of the optional factors up [N, R] / down [R, K] of the norm entry points."""
    if (up is None) != (down is None):
        raise _lib.SdnqHipError(f"{what}: up and down come together (both or neither)")
    if n % 8 or k % 16:
        raise _lib.SdnqHipError(f"{what}: n % 8 == 0 and k % 16 == 0 (got n = {n}, k = {k})")
    if up is None:
        return 0, None
    if up.ndim != 2 or down.ndim != 2:
        raise _lib.SdnqHipError(f"{what}: up and down must be 2-D (got {tuple(up.shape)}, {tuple(down.shape)})")
    r = up.shape[1]
    _lowrank_check(what, r, up=up, down=down)
    if tuple(up.shape) != (n, r) or tuple(down.shape) != (r, k):
        raise _lib.SdnqHipError(f"{what}: up [N, R] and down [R, K] for a weight [{n}, {k}] (got {tuple(up.shape)}, {tuple(down.shape)})")
    if not up.is_contiguous() or not down.is_contiguous():
        raise _lib.SdnqHipError(f"{what}: up and down must be contiguous")
    return r, float_code(up.dtype)


def dora_normsq(qw: QuantWeight, up: torch.Tensor | None = None, down: torch.Tensor | None = None, scale: float = 1.0) -> torch.Tensor:
    """sdnq_hip_dora_normsq: out [N] float32 = sum_k (w32[n][k] + scale * (up @ down)[n][k])^2 from the stored codes of `qw` (no SVD
    factors), each element e = fma(scale, acc, w32) in float32 with the rank sum on the matrix cores; up [N, R] / down [R, K] contiguous,
    bfloat16 / float16, or both None for the plain squared row norms.  One launch, no [N, K] tensor, the same bits on every call."""
    r, code = _dora_factors("dora_normsq", qw.n, qw.k, up, down)
    dev = qw.keep[0].device
    _require_cuda(qw.keep[0], up, down)
    out = torch.empty(qw.n, device=dev, dtype=torch.float32)
    check(_lib.load().sdnq_hip_dora_normsq(ctypes.byref(qw.desc), _ptr(up), _ptr(down), BF16 if code is None else code, r, float(scale),
                                           out.data_ptr(), _stream(out)), "dora_normsq")
    return out


def dora_normsq_dense(wd: torch.Tensor, up: torch.Tensor | None = None, down: torch.Tensor | None = None, scale: float = 1.0) -> torch.Tensor:
    """sdnq_hip_dora_normsq_dense: ``dora_normsq`` on a dense weight wd [N, K] (bfloat16 / float16, unit column stride, 16-byte aligned
    rows) of the factors' dtype: the route of layers with SVD factors or a Hadamard rotation, on what ``dequant`` wrote."""
    if wd.ndim != 2:
        raise _lib.SdnqHipError(f"dora_normsq_dense: wd must be 2-D (got {tuple(wd.shape)})")
    n, k = wd.shape
    r, _ = _dora_factors("dora_normsq_dense", n, k, up, down)
    _lowrank_check("dora_normsq_dense", r or 8, wd=wd, **({} if up is None else {"up": up}))
    _require_cuda(wd, up, down)
    out = torch.empty(n, device=wd.device, dtype=torch.float32)
    check(_lib.load().sdnq_hip_dora_normsq_dense(wd.data_ptr(), float_code(wd.dtype), n, k, _ld(wd), _ptr(up), _ptr(down), r, float(scale),
                                                 out.data_ptr(), _stream(out)), "dora_normsq_dense")
    return out


def _code_buffer(storage: int, bits: int, n: int, k: int, dev) -> torch.Tensor:
    """The flat buffer the quantizer kernels write the codes of an [N, K] weight into."""
    if storage == _lib.ST_PACKED_U8:
        return torch.empty((n * k // 8 * bits,), device=dev, dtype=torch.uint8)
    if storage == _lib.ST_PACKED_I16:
        return torch.empty((n * k // 16 * bits,), device=dev, dtype=torch.int16)
    return torch.empty((n, k), device=dev, dtype=torch.uint8 if storage == _lib.ST_RAW8 else torch.int16)


def _code_view(raw: torch.Tensor, weights_dtype: str) -> torch.Tensor:
    """`raw` shaped and typed as ``quantize_weight`` returns the codes of `weights_dtype`."""
    from . import packed as _packed
    ent = dtype_dict[weights_dtype]
    bits = ent["num_bits"]
    if ent["is_packed"] and bits not in (8, 16):
        _g, words, _wb = _packed._GEOM[bits]
        return raw if words == 1 else raw.view(-1, words)
    if ent["is_packed"]:  # custom float8 / float16 codes (pack_float returns uint8 / uint16)
        return raw.view(torch.uint16) if bits == 16 else raw
    return raw.view(ent["torch_dtype"]) if ent["torch_dtype"].itemsize == raw.element_size() else raw


def _format_fields(storage, kind, bits, ebits, mbits, native) -> tuple:
    """What tells two storage formats apart: a codebook's codes are unsigned integers, and integers have no exponent / mantissa split."""
    kind = _lib.KIND_UINT if kind == _lib.KIND_CODEBOOK else kind
    if kind in (_lib.KIND_INT, _lib.KIND_UINT):
        return storage, kind, bits
    return storage, kind, bits, ebits, mbits, native


def _format_name(d) -> str:
    """The key of ``dtype_dict`` whose storage fields are those of the descriptor `d` (a codebook's: its unsigned integer codes)."""
    want = _format_fields(d.storage, d.kind, d.bits, d.exponent, d.mantissa, d.native_float)
    for name in dtype_dict:
        try:
            if _format_fields(*_storage_kind(name)) == want:
                return name
        except (_lib.SdnqHipError, KeyError):
            continue
    raise _lib.SdnqHipError(f"no weights_dtype has the storage fields {want}")


def merge_lowrank_supported(qw: QuantWeight) -> bool:
    """True where sdnq_hip_merge_lowrank is built for the format of `qw` (else it returns SDNQ_ERR_UNSUPPORTED): no codebook, a Linear
    weight, a group size of 16, 32, 64, 128 or 256 or one scale per row."""
    d = qw.desc
    return d.kind != _lib.KIND_CODEBOOK and d.positions <= 1 and (qw.group_size in (16, 32, 64, 128, 256) or qw.group_size == qw.k)


def merge_lowrank(qw: QuantWeight, up: torch.Tensor | None, down: torch.Tensor | None, scale: float = 1.0,
                  row_scale: torch.Tensor | None = None, weights_dtype: str | None = None):
    """sdnq_hip_merge_lowrank: (codes, scale [N, G] float32, zero_point [N, G] float32 | None) of the re-quantized
    ``row_scale[:, None] * (w32 + scale * up @ down)`` from the stored codes of `qw` in ONE launch -- every element
    e = fma(scale, acc, w32) in float32 (``dora_normsq``'s definitions; SVD factors of `qw` are ignored: the codes are the residual), then
    the arithmetic and the storage of ``quantize_weight`` with the group size of `qw`: the outputs have the shapes and dtypes
    ``quantize_weight`` returns and are its bits on the float32 matrix e.  up [N, R] / down [R, K] contiguous bfloat16 / float16, or both
    None with `row_scale` [N] float32 for a pure row rescale.  `weights_dtype` names the format of `qw` (the key of ``dtype_dict``, whose
    min / max are the clamp; None: found from the descriptor's fields).  ``merge_lowrank_supported(qw)`` says beforehand what the kernel is
    built for; it raises SdnqHipError with status SDNQ_ERR_UNSUPPORTED for what the kernel is not built for (group
    sizes other than 16 .. 256 powers of two and row-wise, codebooks, conv weights): callers compose ``dequant`` + ``quantize_weight``."""
    r, code = _dora_factors("merge_lowrank", qw.n, qw.k, up, down)
    if up is None and row_scale is None:
        raise _lib.SdnqHipError("merge_lowrank: nothing to merge (up, down and row_scale are all None)")
    d0 = qw.desc
    if weights_dtype is None:
        weights_dtype = _format_name(d0)
    ent = dtype_dict[weights_dtype]
    storage, kind, bits, ebits, mbits, native = _storage_kind(weights_dtype)
    if _format_fields(storage, kind, bits, ebits, mbits, native) != _format_fields(d0.storage, d0.kind, d0.bits, d0.exponent, d0.mantissa,
                                                                                   d0.native_float):
        raise _lib.SdnqHipError(f"merge_lowrank: weights_dtype {weights_dtype} is not the format of qw")
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or tuple(row_scale.shape) != (qw.n,) or not row_scale.is_contiguous():
            raise _lib.SdnqHipError(f"merge_lowrank: row_scale must be a contiguous float32 [N] = [{qw.n}] (got {row_scale.dtype} "
                                    f"{tuple(row_scale.shape)})")
    dev = qw.keep[0].device
    _require_cuda(qw.keep[0], up, down, row_scale)
    g = qw.k // qw.group_size
    raw = _code_buffer(storage, bits, qw.n, qw.k, dev)
    sc = torch.empty((qw.n, g), device=dev, dtype=torch.float32)
    zp = torch.empty((qw.n, g), device=dev, dtype=torch.float32) if ent["is_unsigned"] else None
    d = SdnqWeight(weight=raw.data_ptr(), scale=sc.data_ptr(), zero_point=_ptr(zp), svd_up=None, svd_down=None, n=qw.n, k=qw.k,
                   group_size=qw.group_size, svd_rank=0, svd_dtype=0, storage=d0.storage, kind=d0.kind, bits=d0.bits, exponent=d0.exponent,
                   mantissa=d0.mantissa, native_float=d0.native_float, positions=d0.positions)
    check(_lib.load().sdnq_hip_merge_lowrank(ctypes.byref(d0), ctypes.byref(d), _ptr(up), _ptr(down), BF16 if code is None else code, r,
                                             float(scale), _ptr(row_scale), float(ent["min"]), float(ent["max"]), _stream(raw)),
          "merge_lowrank")
    return _code_view(raw, weights_dtype), sc, zp


def _dora_vectors(what: str, n: int, dt: torch.dtype, c: torch.Tensor, bias) -> None:
    if c.dtype != torch.float32 or tuple(c.shape) != (n,) or not c.is_contiguous() or c.data_ptr() % 16:
        raise _lib.SdnqHipError(f"{what}: c must be a contiguous, 16-byte aligned float32 vector [N = {n}] (got {c.dtype}, {tuple(c.shape)})")
    if bias is not None and (bias.dtype != dt or tuple(bias.shape) != (n,) or not bias.is_contiguous() or bias.data_ptr() % 16):
        raise _lib.SdnqHipError(f"{what}: bias must be a contiguous, 16-byte aligned {dt} vector [N = {n}] (got {bias.dtype}, {tuple(bias.shape)})")


def lowrank_add_dora(t: torch.Tensor, up: torch.Tensor, y: torch.Tensor, scale: float, c: torch.Tensor, bias=None) -> torch.Tensor:
    """sdnq_hip_lowrank_add_dora: ``lowrank_add`` with DoRA's epilogue IN PLACE on y [M, N] = the base output z (bias included):
    y = round(fma(c * scale, t @ up^T, fma(c - 1, z - bias, z))), c [N] float32, bias [N] of y's dtype or None.  With c == 1 the bits of
    ``lowrank_add``.  Returns y."""
    return _lowrank_add("lowrank_add_dora", t, up, y, scale, dora=(c, bias))


def dora_bwd_workspace_bytes(m: int, n: int) -> int:
    """sdnq_hip_dora_bwd_workspace_bytes: 0 while the m rows fit one slab of the deterministic reduction."""
    nbytes = _lib.load().sdnq_hip_dora_bwd_workspace_bytes(m, n)
    if nbytes < 0:
        check(int(nbytes), "dora_bwd_workspace_bytes")
    return int(nbytes)


def dora_bwd(dy: torch.Tensor, y: torch.Tensor | None, bias, c: torch.Tensor, want_q: bool = True, workspace: torch.Tensor | None = None):
    """sdnq_hip_dora_bwd: (g, q) in one pass -- g [M, N] = round(dy * c) in dy's dtype, q [N] float32 = sum_i dy[i] * (y[i] - bias) (None
    with want_q=False: y is then not read and may be None).  dy, y: bfloat16 / float16 with unit column stride and 16-byte aligned rows; c
    [N] float32; bias [N] of dy's dtype or None.  Slabs of 256 rows added in a fixed order: the same bits on every call.  workspace as
    ``lowrank_grad``: at least dora_bwd_workspace_bytes(M, N) bytes of uint8, or None for this module's per-stream buffer."""
    what = "dora_bwd"
    if dy.ndim != 2:
        raise _lib.SdnqHipError(f"{what}: dy must be 2-D (got {tuple(dy.shape)})")
    m, n = dy.shape
    ops_t = {"dy": dy}
    if want_q:
        if y is None or tuple(y.shape) != (m, n):
            raise _lib.SdnqHipError(f"{what}: y must have dy's shape {(m, n)} (got {None if y is None else tuple(y.shape)})")
        ops_t["y"] = y
    _lowrank_check(what, 8, **ops_t)
    if n % 8:
        raise _lib.SdnqHipError(f"{what}: n % 8 == 0 (got n = {n}): the rows move in 16-byte pieces")
    _dora_vectors(what, n, dy.dtype, c, bias)
    _require_cuda(dy, y if want_q else None, c, bias, workspace)
    g = torch.empty((m, n), device=dy.device, dtype=dy.dtype)
    q = torch.empty(n, device=dy.device, dtype=torch.float32) if want_q else None
    if m == 0:
        return g, (q.zero_() if want_q else None)
    need = dora_bwd_workspace_bytes(m, n) if want_q else 0
    wp = _grad_workspace(what, dy.device, _stream(dy), need, workspace)
    check(_lib.load().sdnq_hip_dora_bwd(dy.data_ptr(), _ld(dy), y.data_ptr() if want_q else None, _ld(y) if want_q else 0, _ptr(bias),
                                        c.data_ptr(), float_code(dy.dtype), m, n, g.data_ptr(), _ptr(q), wp, need, _stream(dy)), what)
    return g, q


def _conv_lowrank_check(what: str, x: torch.Tensor, other: torch.Tensor, kernel, stride, padding, dilation):
    """The checks the two conv adapter entry points share -- x [B, C, H, W] and a 2-D operand with `rank` rows / columns of ONE 16-bit dtype,
    8 | C kh kw -- and their integer arguments: (geometry tuple of 12 ints, (B, H_out, W_out), K)."""
    if x.ndim != 4 or other.ndim != 2:
        raise _lib.SdnqHipError(f"{what}: x must be [B, C, H, W] and the factor 2-D (got {tuple(x.shape)}, {tuple(other.shape)})")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.SdnqHipError(f"{what}: built for bfloat16 / float16 operands (got {x.dtype})")
    if other.dtype != x.dtype:
        raise _lib.SdnqHipError(f"{what}: the factor must have the dtype of x (got {other.dtype}, {x.dtype})")
    b, c, h, w = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if b <= 0 or c <= 0 or ho <= 0 or wo <= 0:
        raise _lib.SdnqHipError(f"{what}: the convolution output would be empty (x {tuple(x.shape)}, output {ho} x {wo})")
    k = c * kh * kw
    if k % 8:
        raise _lib.SdnqHipError(f"{what}: C * kh * kw % 8 == 0 (got {k}): the factor's rows move in 16-byte pieces")
    return (b, c, h, w, kh, kw, sh, sw, ph, pw, dh, dw), (b, ho, wo), k


def conv_lowrank_down(x: torch.Tensor, down: torch.Tensor, kernel, stride, padding, dilation) -> tuple[torch.Tensor, tuple]:
    """sdnq_hip_conv_lowrank_down: t [B * H_out * W_out, R] = round(im2col(x) @ down [R, C * kh * kw]^T) for x [B, C, H, W] without the
    unfolded matrix: the down projection of a conv adapter (lora_A.weight viewed 2-D), float32 sums on the matrix cores, one launch.
    bfloat16 / float16.  The value of lowrank_down(im2col(x), down) up to the order of the float32 sum.  Returns (t, (B, H_out, W_out))."""
    geo, out_shape, k = _conv_lowrank_check("conv_lowrank_down", x, down, kernel, stride, padding, dilation)
    r = down.shape[0]
    _rank_check("conv_lowrank_down", r)
    if down.shape[1] != k or not down.is_contiguous():
        raise _lib.SdnqHipError(f"conv_lowrank_down: down must be contiguous [R, C * kh * kw = {k}] (got {tuple(down.shape)}, strides {down.stride()})")
    _require_cuda(x, down)
    x = x if x.is_contiguous() else x.contiguous()
    t = torch.empty((out_shape[0] * out_shape[1] * out_shape[2], r), device=x.device, dtype=x.dtype)
    check(_lib.load().sdnq_hip_conv_lowrank_down(x.data_ptr(), float_code(x.dtype), *geo, down.data_ptr(), r, t.data_ptr(), _stream(x)),
          "conv_lowrank_down")
    return t, out_shape


def conv_lowrank_grad_workspace_bytes(x_shape, kernel, stride, padding, dilation, rank: int) -> int:
    """sdnq_hip_conv_lowrank_grad_workspace_bytes: 0 while the B * H_out * W_out positions fit one slab of the deterministic reduction."""
    b, c, h, w = (int(d) for d in x_shape)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    nbytes = _lib.load().sdnq_hip_conv_lowrank_grad_workspace_bytes(b, c, h, w, kh, kw, sh, sw, ph, pw, dh, dw, int(rank))
    if nbytes < 0:
        check(int(nbytes), "conv_lowrank_grad_workspace_bytes")
    return int(nbytes)


def conv_lowrank_grad(x: torch.Tensor, g: torch.Tensor, kernel, stride, padding, dilation, scale: float = 1.0,
                      out_dtype: torch.dtype | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """sdnq_hip_conv_lowrank_grad: round(scale * g [B * H_out * W_out, R]^T @ im2col(x)) -> [R, C * kh * kw] of `out_dtype` (default: the
    operands') for x [B, C, H, W] without the unfolded matrix: the gradient of a conv adapter's down factor.  float32 sums over slabs of
    positions added in a fixed order: the same bits on every call, no atomics.  workspace: as ops.lowrank_grad's (a uint8 tensor of
    conv_lowrank_grad_workspace_bytes(...) bytes, or None for this module's per-(device, stream) buffer)."""
    geo, out_shape, k = _conv_lowrank_check("conv_lowrank_grad", x, g, kernel, stride, padding, dilation)
    m, r = g.shape
    _rank_check("conv_lowrank_grad", r)
    if m != out_shape[0] * out_shape[1] * out_shape[2] or not g.is_contiguous():
        raise _lib.SdnqHipError(f"conv_lowrank_grad: g must be contiguous [B * H_out * W_out = {out_shape[0] * out_shape[1] * out_shape[2]}, R] "
                                f"(got {tuple(g.shape)}, strides {g.stride()})")
    _require_cuda(x, g, workspace)
    x = x if x.is_contiguous() else x.contiguous()
    out_dtype = x.dtype if out_dtype is None else out_dtype
    out = torch.empty((r, k), device=x.device, dtype=out_dtype)
    need = conv_lowrank_grad_workspace_bytes(x.shape, kernel, stride, padding, dilation, r)
    wp = _grad_workspace("conv_lowrank_grad", x.device, _stream(x), need, workspace)
    check(_lib.load().sdnq_hip_conv_lowrank_grad(x.data_ptr(), float_code(x.dtype), *geo, g.data_ptr(), r, float(scale), out.data_ptr(),
                                                 float_code(out_dtype), wp, need, _stream(x)), "conv_lowrank_grad")
    return out


_workspaces: dict = {}


def _workspace(dev: torch.device, stream: int, nbytes: int) -> torch.Tensor:
    """Scratch buffer of sdnq_hip_linear for (device, stream): grown on demand, reused by every layer on that stream (calls on one
    stream are ordered, so a buffer per stream is never used by two calls at once)."""
    key = (dev.index, stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty((max(nbytes, 1 << 20) + 255,), device=dev, dtype=torch.uint8)
        _workspaces[key] = buf
    return buf


def linear_call(mm: int, x2d: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias, out_dtype: torch.dtype, hadamard_group: int = 0,
                svd_down=None, svd_up=None, zp=None, asymmetric: bool = False, w_colsum_scaled=None, pre=None):
    """The whole quantized-matmul forward of one layer through ONE C call (sdnq_hip_linear): row quantization (unless `pre` =
    (xq, xs, rowsum, xrot, xzp) of an earlier call on the same activation is handed in), low-rank product, scaled matmul with every
    epilogue term.  Returns (out [M, N], (xq, xs, rowsum, xrot, xzp)); the intermediates are torch tensors (they may be cached), only the
    low-rank product lives in the per-stream scratch buffer."""
    _require_cuda(x2d, wq, ws, bias, svd_down, svd_up, zp)
    m, k = x2d.shape
    n = wq.shape[0]
    dev = x2d.device
    a = _lib.SdnqLinearArgs()
    a.struct_size = ctypes.sizeof(_lib.SdnqLinearArgs)
    a.mm_dtype, a.x_dtype, a.out_dtype = mm, float_code(x2d.dtype), float_code(out_dtype)
    a.hadamard_group, a.asymmetric = int(hadamard_group), 1 if asymmetric else 0
    a.m, a.n, a.k, a.ldx = m, n, k, x2d.stride(0)
    out = torch.empty((m, n), device=dev, dtype=out_dtype)
    a.x, a.out, a.wq, a.ws = x2d.data_ptr(), out.data_ptr(), wq.data_ptr(), ws.data_ptr()
    if bias is not None:
        bias = bias.contiguous()
        a.bias, a.bias_dtype = bias.data_ptr(), float_code(bias.dtype)
    if svd_up is not None:
        a.svd_down, a.svd_up, a.svd_rank, a.svd_dtype = svd_down.data_ptr(), svd_up.data_ptr(), svd_up.shape[1], float_code(svd_up.dtype)
        if bias is not None and bias.dtype != svd_up.dtype:
            bias = bias.to(svd_up.dtype)  # the [M, N] bias of the reference lives in the svd dtype (linear_int8.py:60)
            a.bias, a.bias_dtype = bias.data_ptr(), float_code(bias.dtype)
    if zp is not None:
        a.zp = zp.data_ptr()
    if asymmetric:
        a.w_colsum_scaled = w_colsum_scaled.data_ptr()
    need_rowsum, need_xrot = zp is not None, svd_up is not None and hadamard_group != 0
    if pre is not None:
        xq, xs, rowsum, xrot, xzp = pre
        a.x_prequantized = 1
    else:
        xq = torch.empty((m, k), device=dev, dtype=_MM_TORCH[mm])
        xs = torch.empty((m, 1), device=dev, dtype=torch.float32)
        rowsum = torch.empty((m,), device=dev, dtype=torch.int32) if need_rowsum else None
        xrot = torch.empty((m, k), device=dev, dtype=x2d.dtype) if need_xrot else None
        xzp = torch.empty((m, 1), device=dev, dtype=torch.float32) if asymmetric else None
    a.xq, a.xs, a.rowsum, a.xrot, a.xzp = xq.data_ptr(), xs.data_ptr(), _ptr(rowsum), _ptr(xrot), _ptr(xzp)
    lib = _lib.load()
    need = ctypes.c_int64(0)
    check(lib.sdnq_hip_linear_workspace_bytes(ctypes.byref(a), ctypes.byref(need)), "linear_workspace_bytes")
    stream = _stream(x2d)
    if need.value > 0:
        # while the stream is being captured the scratch must belong to the graph's memory pool: the shared per-stream buffer may be
        # replaced (and freed) by a later, larger eager call while the captured graph still holds its address (advisor, round 3)
        w = (torch.empty((need.value + 255,), device=dev, dtype=torch.uint8) if torch.cuda.is_current_stream_capturing()
             else _workspace(dev, stream, need.value))
        base = (w.data_ptr() + 255) & ~255
        a.workspace, a.workspace_bytes = base, w.numel() - (base - w.data_ptr())
    check(lib.sdnq_hip_linear(ctypes.byref(a), stream), "linear")
    return out, (xq, xs, rowsum, xrot, xzp)


def unshard_columns(gathered: torch.Tensor, out: torch.Tensor, starts, m0: int = 0) -> torch.Tensor:
    """out[m0 + i][starts[r] + c] = gathered[r][i][c]: the row-major re-assembly of a column-sharded layer's all-gathered output
    (sdnq_hip_unshard_columns).  gathered [W, rows, wmax] (rank-major, slabs padded to the widest), out [M, N] with N = starts[W]."""
    _require_cuda(gathered, out)
    world, rows, wmax = gathered.shape
    arr = (ctypes.c_int64 * (world + 1))(*[int(v) for v in starts])
    check(_lib.load().sdnq_hip_unshard_columns(gathered.data_ptr(), out.data_ptr(), out.element_size(), m0, rows, out.shape[0], wmax,
                                               world, arr, _stream(out)), "unshard_columns")
    return out


def im2col(x: torch.Tensor, kernel, stride, padding, dilation) -> tuple[torch.Tensor, tuple]:
    """F.unfold(x, ...).transpose(1, 2) for x [B, C, H, W] -> ([B * H_out * W_out, C * kh * kw], (B, H_out, W_out));
    HIP replacement of process_conv_input's unfold (layers/conv/forward.py:75)."""
    _require_cuda(x)
    if x.ndim != 4:
        raise _lib.SdnqHipError("im2col expects [B, C, H, W]")
    x = x if x.is_contiguous() else x.contiguous()
    b, c, h, w = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if ho <= 0 or wo <= 0:
        raise _lib.SdnqHipError(f"convolution output would be empty ({ho} x {wo})")
    out = torch.empty((b * ho * wo, c * kh * kw), device=x.device, dtype=x.dtype)
    check(_lib.load().sdnq_hip_im2col(x.data_ptr(), float_code(x.dtype), b, c, h, w, kh, kw, sh, sw, ph, pw, dh, dw, out.data_ptr(),
                                      _stream(x)), "im2col")
    return out, (b, ho, wo)


def im2col_bwd(dy: torch.Tensor, in_hw, kernel, stride, padding, dilation, row0: int = 0, rows: int | None = None,
               out: torch.Tensor | None = None, groups: int = 1) -> torch.Tensor:
    """sdnq_hip_im2col_bwd: dy [B, C_out, H_out, W_out] gathered per INPUT pixel into rows row0 .. row0 + rows of
    U [B * H * W, kh * kw * C_out] -- the activation operand of grad_x = U . W^T for a conv of this geometry on an input of in_hw = (H, W).
    Columns are (kernel position, channel) -- (group, kernel position, channel inside the group) for groups > 1 -- and a tap that no output
    position matches is 0.  rows=None: everything from row0 on.  out: a 1-D or 2-D tensor of dy's dtype with at least rows * kh * kw * C_out
    elements (its first rows * kh * kw * C_out are written); returned as the [rows, kh * kw * C_out] view."""
    _require_cuda(dy, out)
    if dy.ndim != 4:
        raise _lib.SdnqHipError("im2col_bwd expects grad_output as [B, C_out, H_out, W_out]")
    dy = dy if dy.is_contiguous() else dy.contiguous()
    b, c, ho, wo = dy.shape
    (h, w), (kh, kw), (sh, sw), (ph, pw), (dh, dw) = in_hw, kernel, stride, padding, dilation
    total = b * int(h) * int(w)
    if rows is None:
        rows = total - row0
    kc = kh * kw * c
    if out is None:
        out = torch.empty((rows, kc), device=dy.device, dtype=dy.dtype)
    elif out.dtype != dy.dtype or out.numel() < rows * kc or not out.is_contiguous():
        raise _lib.SdnqHipError(f"im2col_bwd: out must hold {rows * kc} contiguous elements of {dy.dtype}")
    check(_lib.load().sdnq_hip_im2col_bwd(dy.data_ptr(), float_code(dy.dtype), b, c, ho, wo, int(h), int(w), kh, kw, sh, sw, ph, pw, dh, dw,
                                          int(groups), int(row0), int(rows), out.data_ptr(), _stream(dy)), "im2col_bwd")
    return out.view(-1)[:rows * kc].view(rows, kc)


# per (device, stream): [zeroed int32 buffer (ticket + amax map) of sdnq_hip_im2col_rowquant_z, call-in-flight flag]
_amax_maps: dict = {}
_capture_amax_maps: dict = {}  # per (device, stream): (capture id, the map the convs of that capture address)
_AMAX_HEADER = 32 + 256 * 32  # ticket words in front of the map (csrc/conv.hip: SDNQ_CONV_WS_HEADER_WORDS)
SELF_CLEANING_AMAX = os.environ.get("SDNQ_HIP_CONV_SELF_CLEAN", "1") != "0"


def _zeroed_amax_map(x: torch.Tensor, words: int):
    """The stream's self-cleaning amax map, at least _AMAX_HEADER + `words` words, or None (then the caller takes the zero-per-call form): a new
    buffer cannot be made while the stream is capturing (its zero fill would be replayed, its memory would belong to the graph)."""
    if torch.cuda.is_current_stream_capturing():
        # never bake the stream's persistent map into a graph: a graph replayed on ANOTHER stream, beside eager convs on the capture stream,
        # would share one map and one set of tickets with no ordering between them (advisor, round 4).  A captured conv addresses a map of
        # ITS capture: made by the capture's first conv out of the graph's own pool -- its zero fill is part of the graph, ONE zeroing launch
        # per replay -- and kept all-zero between the graph's convs by the self-cleaning kernel (round 5: the zero-per-call form cost a
        # captured SDXL conv step 48 launches of 5 us, 8 % of it).
        cid = ctypes.c_uint64(0)
        check(_lib.load().sdnq_hip_stream_capture_id(_stream(x), ctypes.byref(cid)), "stream_capture_id")
        if cid.value == 0:
            return None
        key = (x.device.index, _stream(x))
        cap = _capture_amax_maps.get(key)
        need = _AMAX_HEADER + words
        if cap is None or cap[0] != cid.value or cap[1].numel() < need:
            cap = (cid.value, torch.zeros((max(need, _AMAX_HEADER + 65536),), device=x.device, dtype=torch.int32))
            _capture_amax_maps[key] = cap  # (the previous capture's map goes back to ITS graph's pool; that graph keeps addressing it)
        return [cap[1], False]
    key = (x.device.index, _stream(x))
    ent = _amax_maps.get(key)
    need = _AMAX_HEADER + words
    if ent is None or ent[0].numel() < need or ent[1]:
        if ent is not None and ent[0].numel() >= need:  # a call that failed midway may have left marks behind
            ent[0].zero_()
            ent[1] = False
        else:  # (an outgrown map is simply dropped: no graph holds its address, and the stream orders its last use before the free)
            ent = [torch.zeros((max(need, _AMAX_HEADER + 65536),), device=x.device, dtype=torch.int32), False]
            _amax_maps[key] = ent
    return ent


def im2col_rowquant(x: torch.Tensor, kernel, stride, padding, dilation, mm: int):
    """Fused unfold + row-wise activation quantization for the conv matmul forwards:
    -> (xq [M, K] int8 | fp8, xs [M, 1] f32, (B, H_out, W_out)); equals rowquant(im2col(x))."""
    _require_cuda(x)
    if x.ndim != 4:
        raise _lib.SdnqHipError("im2col_rowquant expects [B, C, H, W]")
    x = x if x.is_contiguous() else x.contiguous()
    b, c, h, w = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, padding, dilation
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if ho <= 0 or wo <= 0:
        raise _lib.SdnqHipError(f"convolution output would be empty ({ho} x {wo})")
    m, k = b * ho * wo, c * kh * kw
    xq = torch.empty((m, k), device=x.device, dtype=_MM_TORCH[mm])
    xs = torch.empty((m, 1), device=x.device, dtype=torch.float32)
    ent = _zeroed_amax_map(x, b * h * w) if SELF_CLEANING_AMAX else None
    if ent is not None:  # the stream's persistent map: zero on entry, zeroed again by the quantizing kernel's last workgroup
        ent[1] = True
        check(_lib.load().sdnq_hip_im2col_rowquant_z(x.data_ptr(), float_code(x.dtype), b, c, h, w, kh, kw, sh, sw, ph, pw, dh, dw, mm,
                                                     xq.data_ptr(), xs.data_ptr(), ent[0].data_ptr(), _stream(x)), "im2col_rowquant_z")
        ent[1] = False
        return xq, xs, (b, ho, wo)
    ws = torch.empty((b * h * w,), device=x.device, dtype=torch.int32)  # per-pixel channel-amax map (zeroed by the library)
    check(_lib.load().sdnq_hip_im2col_rowquant(x.data_ptr(), float_code(x.dtype), b, c, h, w, kh, kw, sh, sw, ph, pw, dh, dw, mm,
                                               xq.data_ptr(), xs.data_ptr(), ws.data_ptr(), _stream(x)), "im2col_rowquant")
    return xq, xs, (b, ho, wo)


def quantize_codebook(weight2d: torch.Tensor, weights_dtype: str, group_size: int, positions: int = 1, steps: int = 24):
    """Float [N,K] weight -> (codes, levels f32 [N, G, L, P]) of the codebook quantizer (sdnq_hip_quantize_codebook; the reference's
    quantize_weight_codebook + pack_int): codes packed like `quantize_weight` returns them ([N,K] uint8 for uint8).  `group_size`
    == K / P for one slice per row; positions as in `quantize_weight`."""
    from .common import dtype_dict
    from . import packed as _packed
    _require_cuda(weight2d)
    if weight2d.dtype not in _FLOAT_CODE:
        raise _lib.SdnqHipError(f"quantize_codebook: unsupported source dtype {weight2d.dtype}")
    w = weight2d if weight2d.stride(1) == 1 else weight2d.contiguous()
    n, k = w.shape
    storage, kind, bits, _, _, _ = _storage_kind(weights_dtype)
    if kind != _lib.KIND_UINT or bits > 8:
        raise _lib.SdnqHipError(f"codebook quantization is only supported with unsigned integer dtypes of up to 8 bits (got {weights_dtype})")
    g = (k // positions) // group_size
    dev = w.device
    raw = torch.empty((n, k), device=dev, dtype=torch.uint8) if bits == 8 else torch.empty((n * k // 8 * bits,), device=dev, dtype=torch.uint8)
    levels = torch.empty((n, g, 1 << bits, positions), device=dev, dtype=torch.float32)
    d = SdnqWeight(weight=raw.data_ptr(), scale=levels.data_ptr(), zero_point=None, svd_up=None, svd_down=None, n=n, k=k,
                   group_size=group_size, svd_rank=0, svd_dtype=0, storage=storage, kind=_lib.KIND_CODEBOOK, bits=bits, exponent=0,
                   mantissa=0, native_float=0, positions=positions)
    check(_lib.load().sdnq_hip_quantize_codebook(w.data_ptr(), float_code(w.dtype), w.stride(0), ctypes.byref(d), int(steps), _stream(w)),
          "quantize_codebook")
    if bits != 8:
        _g, words, _wb = _packed._GEOM[bits]
        raw = raw if words == 1 else raw.view(-1, words)
    return raw, levels


def quantize_weight(weight2d: torch.Tensor, weights_dtype: str, group_size: int, positions: int = 1):
    """Float [N,K] weight -> (codes, scale [N,G] f32, zero_point [N,G] f32 | None) with the codes in the reference's storage
    (packed words shaped like the reference's packers return them, or [N,K] raw int8/uint8/int16/fp8/fp16...).
    HIP replacement of quantize_weight + pack_int / pack_float (quant_utils.py:28-56, packed_int/__init__.py:77-80,
    packed_float.py:27-82); `group_size` == K for row-wise.  positions = P > 1: conv weight flattened to [N, C_in * P],
    group_size counts channels, scales are [N, (C_in / group_size) * P]."""
    _require_cuda(weight2d)
    if weight2d.dtype not in _FLOAT_CODE:
        raise _lib.SdnqHipError(f"quantize_weight: unsupported source dtype {weight2d.dtype}")
    w = weight2d if weight2d.stride(1) == 1 else weight2d.contiguous()
    n, k = w.shape
    ent = dtype_dict[weights_dtype]
    storage, kind, bits, ebits, mbits, native = _storage_kind(weights_dtype)
    g = (k // positions) // group_size * positions
    dev = w.device
    raw = _code_buffer(storage, bits, n, k, dev)
    scale = torch.empty((n, g), device=dev, dtype=torch.float32)
    zp = torch.empty((n, g), device=dev, dtype=torch.float32) if ent["is_unsigned"] else None
    d = SdnqWeight(weight=raw.data_ptr(), scale=scale.data_ptr(), zero_point=_ptr(zp), svd_up=None, svd_down=None, n=n, k=k,
                   group_size=group_size, svd_rank=0, svd_dtype=0, storage=storage, kind=kind, bits=bits, exponent=ebits,
                   mantissa=mbits, native_float=native, positions=positions)
    check(_lib.load().sdnq_hip_quantize_weight(w.data_ptr(), float_code(w.dtype), w.stride(0), ctypes.byref(d), float(ent["min"]),
                                               float(ent["max"]), _stream(w)), "quantize_weight")
    return _code_view(raw, weights_dtype), scale, zp


def _adamw_tail(p: torch.Tensor, lr, betas, step, weight_decay, clip, grad_scale, sr_param, sr_state, seed, offset):
    """The scalar arguments the two AdamW entry points share: Python doubles here, rounded to float32 by the binding, as torch
    rounds a Python scalar that meets a float32 tensor."""
    b1, b2 = betas
    decay = 1.0 - lr * weight_decay if weight_decay != 0 else 1.0
    return (float(lr), 1.0 - b1, 1.0 - b2, 1.0 - b1 ** step, 1.0 - b2 ** step, float(clip), decay, _ptr(grad_scale),
            int(bool(sr_param)), int(bool(sr_state)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, _stream(p))


def _adamw_check(p: torch.Tensor, g: torch.Tensor, grad_scale) -> None:
    _require_cuda(p, g, grad_scale)
    if g.dtype != p.dtype or g.shape != p.shape:
        raise _lib.SdnqHipError(f"adamw_step: grad must have the parameter's dtype and shape (got {g.dtype} {tuple(g.shape)} for "
                                f"{p.dtype} {tuple(p.shape)})")
    if not p.is_contiguous() or not g.is_contiguous():
        raise _lib.SdnqHipError("adamw_step: param and grad must be contiguous")
    if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.numel() != 1):
        raise _lib.SdnqHipError("adamw_step: grad_scale must be one float32 element on the device")


def _adamw_dense_state(p: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor) -> list:
    """The addresses of dense state, checked against its parameter."""
    for t in (exp_avg, exp_avg_sq):
        _require_cuda(t)
        if t.dtype != p.dtype or t.numel() != p.numel() or not t.is_contiguous():
            raise _lib.SdnqHipError("adamw_step: dense state must be contiguous, of the parameter's dtype and size")
    return [exp_avg.data_ptr(), exp_avg_sq.data_ptr()]


def _adamw_q8_state(p: torch.Tensor, exp_avg, exp_avg_sq) -> list:
    """The six addresses of uint8 state (codes, scale, zero point of either moment), checked against its parameter."""
    ptrs = []
    for q, s, z in (exp_avg, exp_avg_sq):
        _require_cuda(q, s, z)
        if (q.dtype != torch.uint8 or q.numel() != p.numel() or s.dtype != torch.float32 or z.dtype != torch.float32
                or s.numel() * 32 != p.numel() or z.numel() != s.numel() or not (q.is_contiguous() and s.is_contiguous() and z.is_contiguous())):
            raise _lib.SdnqHipError("adamw_step_q8: state must be contiguous uint8 codes [numel] with float32 scale and zero point [numel / 32]")
        ptrs += [q.data_ptr(), s.data_ptr(), z.data_ptr()]
    return ptrs


def adamw_step(p: torch.Tensor, g: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, *, step: int, lr: float,
               betas=(0.9, 0.999), weight_decay: float = 0.01, clip: float = 1.0, grad_scale: torch.Tensor | None = None,
               sr_param: bool = False, sr_state: bool = False, seed: int = 0, offset: int = 0) -> None:
    """sdnq_hip_adamw_step: one fused AdamW update of `p` in place, with dense state in p's dtype.  `step` counts from 1."""
    _adamw_check(p, g, grad_scale)
    state = _adamw_dense_state(p, exp_avg, exp_avg_sq)
    check(_lib.load().sdnq_hip_adamw_step(p.data_ptr(), g.data_ptr(), *state, float_code(p.dtype),
                                          p.numel(), *_adamw_tail(p, lr, betas, step, weight_decay, clip, grad_scale, sr_param,
                                                                  sr_state, seed, offset)), "adamw_step")


def adamw_step_q8(p: torch.Tensor, g: torch.Tensor, exp_avg, exp_avg_sq, *, step: int, lr: float, betas=(0.9, 0.999),
                  weight_decay: float = 0.01, clip: float = 1.0, grad_scale: torch.Tensor | None = None, sr_param: bool = False,
                  sr_state: bool = False, seed: int = 0, offset: int = 0) -> None:
    """sdnq_hip_adamw_step_q8: the same with uint8 state; exp_avg / exp_avg_sq are (codes uint8 [numel], scale f32 [numel / 32],
    zero_point f32 [numel / 32]) triples, updated in place."""
    _adamw_check(p, g, grad_scale)
    ptrs = _adamw_q8_state(p, exp_avg, exp_avg_sq)
    check(_lib.load().sdnq_hip_adamw_step_q8(p.data_ptr(), g.data_ptr(), float_code(p.dtype), p.numel(), *ptrs,
                                             *_adamw_tail(p, lr, betas, step, weight_decay, clip, grad_scale, sr_param, sr_state,
                                                          seed, offset)), "adamw_step_q8")


def _adamw_multi(entry: str, state_of, params, grads, exp_avgs, exp_avg_sqs, steps, offsets, lr, betas, weight_decay, clip, grad_scale,
                 sr_param, sr_state, seed) -> None:
    """One call of a multi-tensor entry point: the single-tensor checks per tensor, the addresses column by column as host arrays, and
    _adamw_tail's scalars -- bc1 and bc2 once per distinct step, everything else shared."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(steps) == len(offsets) == n):
        raise _lib.SdnqHipError(f"{entry}: params, grads, exp_avgs, exp_avg_sqs, steps and offsets must have one entry per tensor")
    if n == 0:
        return
    rows = []
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        if p.dtype != params[0].dtype or p.device != params[0].device:
            raise _lib.SdnqHipError(f"{entry}: the tensors of one call must share a dtype and a device (got {p.dtype} on {p.device} "
                                    f"beside {params[0].dtype} on {params[0].device})")
        _adamw_check(p, g, grad_scale)
        rows.append([p.data_ptr(), g.data_ptr(), *state_of(p, m, v)])
    tails = {s: _adamw_tail(params[0], lr, betas, s, weight_decay, clip, grad_scale, sr_param, sr_state, seed, 0) for s in set(steps)}
    lr_, w1, w2, _bc1, _bc2, clip_, decay, gs, srp, srs, seed_, _offset, stream = tails[steps[0]]
    columns = [(ctypes.c_void_p * n)(*column) for column in zip(*rows)]
    check(getattr(_lib.load(), entry)(
        n, *columns, (ctypes.c_int64 * n)(*(p.numel() for p in params)), (ctypes.c_float * n)(*(tails[s][3] for s in steps)),
        (ctypes.c_float * n)(*(tails[s][4] for s in steps)), (ctypes.c_uint64 * n)(*(int(o) & 0xFFFFFFFFFFFFFFFF for o in offsets)),
        float_code(params[0].dtype), lr_, w1, w2, clip_, decay, gs, srp, srs, seed_, stream), entry[len("sdnq_hip_"):])


def adamw_step_multi(params, grads, exp_avgs, exp_avg_sqs, *, steps, offsets, lr: float, betas=(0.9, 0.999), weight_decay: float = 0.01,
                     clip: float = 1.0, grad_scale: torch.Tensor | None = None, sr_param: bool = False, sr_state: bool = False,
                     seed: int = 0) -> None:
    """sdnq_hip_adamw_step_multi: adamw_step on every (params[i], grads[i], exp_avgs[i], exp_avg_sqs[i]) with step steps[i] and random
    offset offsets[i], bit for bit, in one launch per sdnq_hip_adamw_multi_capacity(0) tensors.  One dtype and one device per call."""
    _adamw_multi("sdnq_hip_adamw_step_multi", _adamw_dense_state, params, grads, exp_avgs, exp_avg_sqs, steps, offsets, lr, betas,
                 weight_decay, clip, grad_scale, sr_param, sr_state, seed)


def adamw_step_multi_q8(params, grads, exp_avgs, exp_avg_sqs, *, steps, offsets, lr: float, betas=(0.9, 0.999),
                        weight_decay: float = 0.01, clip: float = 1.0, grad_scale: torch.Tensor | None = None, sr_param: bool = False,
                        sr_state: bool = False, seed: int = 0) -> None:
    """sdnq_hip_adamw_step_multi_q8: the same on adamw_step_q8; exp_avgs[i] / exp_avg_sqs[i] are its (codes, scale, zero_point) triples."""
    _adamw_multi("sdnq_hip_adamw_step_multi_q8", _adamw_q8_state, params, grads, exp_avgs, exp_avg_sqs, steps, offsets, lr, betas,
                 weight_decay, clip, grad_scale, sr_param, sr_state, seed)
