"""ONE predicate for "does the MI355X path compute this layer": `unsupported_reason(module)`.

`accelerate()` asks it per module BEFORE re-pointing anything: a layer the HIP forwards do not build keeps the `forward_func` it
came with (a reference-built model keeps working on the reference's own forward for that layer -- the reference's idiom for a
missing kernel is fall back + log.warning, kernel_wrappers.py:80-88), and one `warnings.warn` lists what was left alone.  The
forwards ask the same function when they build a layer's kernel state (`linear._state`), so the two can never disagree: a layer
quantized by THIS package in an unbuilt configuration still fails loudly, with the same sentence.

Only STATIC facts of the module are judged here (configuration, stored dtypes, conv geometry); what depends on the call (input
dtype / device) stays in the forwards.
"""
from __future__ import annotations

import torch

from .common import conv_transpose_types, conv_types, dtype_dict, embedding_types, linear_types


def _scale_dtype(module):
    sc = getattr(module, "scale", None)
    return None if sc is None else sc.dtype


def unsupported_reason(module) -> str | None:
    """None when the HIP forwards compute `module` (an SDNQ-quantized layer); otherwise the sentence that says why not."""
    dq = getattr(module, "sdnq_dequantizer", None)
    if dq is None:
        return "not an SDNQ layer (no sdnq_dequantizer)"
    cls = getattr(dq, "layer_class_name", None)
    if cls in conv_transpose_types:
        return _conv_transpose_reason(module, dq, cls)
    if cls not in linear_types and cls not in conv_types and cls not in embedding_types:
        return f"{cls}: unknown layer class"
    if dq.weights_dtype not in dtype_dict or dq.quantized_matmul_dtype not in dtype_dict:
        return f"unknown dtype {dq.weights_dtype} / {dq.quantized_matmul_dtype}"
    if getattr(dq, "use_codebook", False):
        why = _codebook_reason(dq, cls)
        if why is not None:
            return why
    mm = dtype_dict[dq.quantized_matmul_dtype]
    qmm = bool(dq.use_quantized_matmul)
    sdt = _scale_dtype(module)
    lp = sdt is not None and sdt not in (torch.float32, torch.float64)
    if cls in embedding_types:
        return _embedding_reason(module, dq, sdt, lp)
    if lp and sdt != dq.result_dtype:
        return (f"scale dtype {sdt} differs from the layer's result dtype {dq.result_dtype}: 16-bit scales are built for the layout "
                "apply_sdnq_options_to_model(dequantize_fp32=False) produces")
    if qmm and not mm["is_integer"] and mm["num_bits"] != 8:
        # the float16 matmul (linear_fp16.py; round 6) is built for Linear layers: stored float codes or weights re-quantized to float16 codes,
        # with Hadamard rotation and SVD factors
        if dq.quantized_matmul_dtype != "float16" or cls not in linear_types:
            return f"quantized_matmul_dtype='{dq.quantized_matmul_dtype}' on {cls} is outside the MI355X hot path (SURVEY 8a note)"
        if lp:
            return "the float16 matmul with 16-bit scales (dequantize_fp32=False) is not built"
    w = dtype_dict[dq.weights_dtype]
    if lp and w["num_bits"] > 8:
        return "16-bit scales with formats wider than 8 bits are not built (the codes are not exact in the scale dtype)"
    uint8_mm = qmm and mm["is_integer"] and mm["is_unsigned"]
    if uint8_mm and lp:
        if sdt != torch.bfloat16:
            return ("the uint8 matmul with float16 scales is not built: the reference's float16 column sums (linear_uint8.py:63) overflow "
                    "from K = 512 on")
        if cls not in linear_types and int(getattr(module, "groups", 1)) != 1:
            return "the grouped uint8 conv matmul with 16-bit scales (dequantize_fp32=False) is not built"
    if cls in linear_types:
        return None
    # ---- conv layers
    groups = int(getattr(module, "groups", 1))
    if isinstance(getattr(module, "padding", 0), str):
        return "string padding modes ('same' / 'valid') are not supported by the reference's conv matmul either"
    nd = len(dq.original_shape) - 2
    if nd == 3:
        d = getattr(module, "dilation", (1, 1, 1))
        d = (d,) * 3 if isinstance(d, int) else tuple(d)
        if not (d[0] == d[1] == d[2]):
            return "Conv3d with unequal dilations: the reference's unfold sizes every axis with dilation[0] (forward.py:62-64)"
    if qmm and dq.is_packed and not dq.re_quantize_for_matmul:
        return "packed conv weights with a direct quantized matmul have no valid layout in the reference"
    if uint8_mm and getattr(module, "svd_up", None) is not None:
        return "the uint8 conv matmul with SVD factors is not built (its K * xzp * wzp term is rounded in the conv forwards' own order)"
    if groups != 1:
        if qmm:
            # K per group and N from original_shape, NOT from this package's in_features / out_features properties: the predicate runs on
            # the dequantizer a model CAME with -- the reference's dataclass has no such properties -- before anything is adopted
            k_group = 1
            for d in tuple(dq.original_shape)[1:]:  # original_shape[1] is C_in / groups
                k_group *= int(d)
            k_total, n = k_group * groups, int(dq.original_shape[0])
            if k_total % groups or n % groups or (k_total // groups) % 16 or (n // groups) % 8:
                return f"grouped conv matmul needs 16 | K per group and 8 | channels per group (got {k_total // groups}, {n // groups})"
            if getattr(module, "svd_up", None) is not None:
                return "grouped conv with SVD: the reference's per-group matmul has no valid form for it (its SVD product does not match the grouped weight)"
            if lp and (sdt != torch.bfloat16 or uint8_mm
                       or (getattr(module, "zero_point", None) is not None and not dq.re_quantize_for_matmul)):
                return ("grouped conv matmul with 16-bit scales is built for bfloat16 scales on the int8 / fp8 matmul without a weight zero point (float16: the reference "
                        "casts acc * input_scale to float16 before the weight scale, dequantizer.py:27, 63 -- an epilogue of its own)")
    return None


def _conv_transpose_reason(module, dq, cls) -> str | None:
    """Transposed convolutions (conv_transpose.py): dequantize into the GEMM operand (sdnq_hip_dequant_convt), a float GEMM per conv group
    with a float32 store, one col2im launch.  Plain quantized weights in every storage format, column scales or the square grouped layout,
    float32 scales or the 16-bit ones of apply_sdnq_options_to_model(dequantize_fp32=False)."""
    if dq.weights_dtype not in dtype_dict:
        return f"unknown dtype {dq.weights_dtype}"
    if getattr(dq, "use_codebook", False):
        return f"codebooks on transposed convolutions ({cls}) are not built"
    if getattr(module, "svd_up", None) is not None or getattr(module, "svd_down", None) is not None:
        return f"SVD factors on transposed convolutions ({cls}) are not built"
    if getattr(dq, "use_hadamard", False):
        return f"Hadamard rotation on transposed convolutions ({cls}) is not built"
    if isinstance(getattr(module, "padding", 0), str) or getattr(module, "padding_mode", "zeros") != "zeros":
        return f"string or non-zero padding modes on transposed convolutions ({cls}) are not built (torch's own ConvTransposeNd takes 'zeros' only)"
    if dq.result_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return f"transposed-conv result dtype {dq.result_dtype} is not built (float32, bfloat16, float16 are)"
    sdt = _scale_dtype(module)
    lp = sdt is not None and sdt not in (torch.float32, torch.float64)
    if lp and sdt != dq.result_dtype:
        return (f"scale dtype {sdt} differs from the layer's result dtype {dq.result_dtype}: 16-bit scales are built for the layout "
                "apply_sdnq_options_to_model(dequantize_fp32=False) produces")
    if sdt == torch.float64:
        return "float64 scales on transposed convolutions are not built"
    if lp and dtype_dict[dq.weights_dtype]["num_bits"] > 8:
        return "16-bit scales with formats wider than 8 bits are not built (the codes are not exact in the scale dtype)"
    shape = tuple(int(d) for d in dq.original_shape)
    if len(shape) not in (3, 4, 5):
        return f"transposed-conv weight of shape {shape}: [C_in, C_out / groups, *kernel] with 1 to 3 kernel axes is expected"
    groups = int(getattr(module, "groups", 1))
    p_cols = 1
    for d in shape[1:]:
        p_cols *= d
    if groups < 1 or shape[0] % groups or (shape[0] // groups) % 16:
        return f"transposed conv needs 16 | C_in / groups (got C_in = {shape[0]}, groups = {groups}): the float GEMM's K"
    if p_cols % 16:
        return (f"transposed conv needs 16 | C_out / groups * prod(kernel) (got {p_cols}): the weight kernel decodes 16-element runs of a "
                "stored row")
    return None


def _codebook_reason(dq, cls) -> str | None:
    """use_codebook layers: the codes index a level table per (row, group) that every weight-side kernel gathers from (dequant16)."""
    w = dtype_dict[dq.weights_dtype]
    if not (w["is_integer"] and w["is_unsigned"]):
        return f"codebook quantization is only supported with unsigned integer dtypes (got {dq.weights_dtype})"
    if w["num_bits"] > 8:
        return f"codebooks wider than 8 bits are not built (got {dq.weights_dtype})"
    if int(dq.group_size) == -2:
        return "tensorwise codebooks (group_size=-2) are not built"
    if not dq.re_quantize_for_matmul and dq.use_quantized_matmul:
        return "a codebook layer whose codes feed the matmul directly has no form in the reference (use_codebook re-quantizes)"
    if cls in conv_types and dq.use_quantized_matmul and int(dq.group_size) <= 0:
        return ("an ungrouped codebook conv with a quantized matmul fails in the reference's own forward (its result_shape is None); "
                "grouped codebook convs are built")
    if dq.use_quantized_matmul and dq.quantized_matmul_dtype in ("float16", "fp16"):
        return "the float16 matmul of codebook layers is not built (int8, fp8 and uint8 are)"
    return None


def _embedding_reason(module, dq, sdt, lp) -> str | None:
    """The gather-dequantize kernel (sdnq_hip_embedding) takes a [V, D] table with D % 16 == 0 in every storage format of
    sdnq_hip_dequant, float32 / bfloat16 / float16 results and SVD factors, and Hadamard groups of 4 .. 512."""
    shape = tuple(int(d) for d in dq.original_shape)
    if len(shape) != 2:
        return f"embedding weight of shape {shape}: a [num_embeddings, embedding_dim] table is expected"
    if shape[1] % 16:
        return f"embedding_dim {shape[1]} is not a multiple of 16 (the gather kernel reads 16-element runs of a row)"
    if dq.result_dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return f"embedding result dtype {dq.result_dtype} is not built (float32, bfloat16, float16 are)"
    if sdt is not None and sdt not in (torch.float32, dq.result_dtype):
        return (f"scale dtype {sdt} differs from the layer's result dtype {dq.result_dtype}: 16-bit scales are built for the layout "
                "apply_sdnq_options_to_model(dequantize_fp32=False) produces")
    if lp and dtype_dict[dq.weights_dtype]["num_bits"] > 8:
        return "16-bit scales with formats wider than 8 bits are not built (the codes are not exact in the scale dtype)"
    up = getattr(module, "svd_up", None)
    if up is not None and up.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return f"svd factors in {up.dtype} are not built"
    if dq.use_hadamard:
        g = int(dq.hadamard_group_size)
        if g < 4 or g > 512 or g & (g - 1) or shape[1] % g:
            return f"Hadamard group {g} on embedding_dim {shape[1]}: the fused rotation takes powers of two in [4, 512] dividing the row"
    return None


def require(module) -> None:
    """The forwards' side of the contract: raise the predicate's sentence."""
    why = unsupported_reason(module)
    if why is not None:
        raise NotImplementedError(why)
