"""What the transposed-conv tests share: the fixtures of tests/golden/make_golden_convt.py as tensors, the float layer and the SDNQ module a
fixture describes, and the float64 restatement of its forward (computed once per fixture, never modified)."""
import functools
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NAMES = ["2d_int8_bf16", "2d_sq_uint4_grouped_f16", "2d_k2s2_uint8_f32", "2d_groups2_int8_bf16", "2d_dil_outsize_f16", "1d_fp8_bf16",
         "3d_int8_nobias_bf16", "2d_int5_bf16", "2d_int8_lpscale_bf16"]
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CTOR = {1: torch.nn.ConvTranspose1d, 2: torch.nn.ConvTranspose2d, 3: torch.nn.ConvTranspose3d}
FUNC = {1: torch.nn.functional.conv_transpose1d, 2: torch.nn.functional.conv_transpose2d, 3: torch.nn.functional.conv_transpose3d}
DEQ_KEYS = ["weights_dtype", "quantized_matmul_dtype", "hadamard_group_size", "group_size", "svd_rank", "use_quantized_matmul",
            "re_quantize_for_matmul", "use_hadamard", "use_codebook", "is_packed", "is_unsigned", "is_integer", "is_integer_matmul",
            "layer_class_name"]


def _from_np(arr, tag):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    view = {"bf16": torch.bfloat16, "f16": torch.float16, "fp8e4m3": torch.float8_e4m3fn}
    return t.view(view[tag]) if tag in view else t


@functools.lru_cache(maxsize=None)
def load(name):
    """(meta, {key: tensor}) of fixture `name`; treat the tensors as read-only."""
    with open(os.path.join(GOLDEN, f"convt_{name}.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, f"convt_{name}.npz"))
    return meta, {k: _from_np(z[k], i["dtype"]).reshape(i["shape"]) for k, i in meta["tensors"].items()}


def layer_kwargs(meta):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["layer"].items()}


def float_layer(meta, t):
    """The float ConvTransposeNd the fixture was quantized from."""
    layer = CTOR[meta["nd"]](meta["cin"], meta["cout"], meta["k"], **layer_kwargs(meta)).to(TORCH_DT[meta["dtype"]])
    with torch.no_grad():
        layer.weight.copy_(t["w_float"])
        if "bias" in t:
            layer.bias.copy_(t["bias"])
    return layer


def deq_fields(dq):
    d = {k: getattr(dq, k) for k in DEQ_KEYS}
    d["result_dtype"] = str(dq.result_dtype).replace("torch.", "")
    d["result_shape"] = list(dq.result_shape) if dq.result_shape is not None else None
    d["quantized_weight_shape"] = list(dq.quantized_weight_shape)
    d["original_shape"] = list(dq.original_shape)
    return d


def quantize_here(meta, t, device=None):
    """The fixture's float layer through THIS package's quantizer (and, for the 16-bit-scale fixture, its option application)."""
    import sdnq_amd
    layer = float_layer(meta, t)
    if device is not None:
        layer = layer.to(device)
    q = sdnq_amd.sdnq_quantize_layer(layer, sdnq_amd.SDNQConfig(**meta["cfg"]))[0]
    if meta["lpscale"]:
        sdnq_amd.apply_sdnq_options_to_model(torch.nn.Sequential(q), dequantize_fp32=False)
    return q


def stored_module(meta, t, device=None):
    """The SDNQ module of the fixture's STORED tensors (what a loader rebuilds), on `device`."""
    from sdnq_amd.dequantizer import SDNQDequantizer
    from sdnq_amd.forward import get_forward_func
    from sdnq_amd.layers import get_sdnq_wrapper_class
    d = meta["deq"]
    layer = float_layer(meta, t)
    layer.sdnq_dequantizer = SDNQDequantizer(
        result_dtype=TORCH_DT[meta["dtype"]], result_shape=None if d["result_shape"] is None else torch.Size(d["result_shape"]),
        original_shape=torch.Size(d["original_shape"]), original_stride=list(t["w_float"].stride()),
        quantized_weight_shape=torch.Size(d["quantized_weight_shape"]), weights_dtype=d["weights_dtype"],
        quantized_matmul_dtype=d["quantized_matmul_dtype"], hadamard_group_size=d["hadamard_group_size"], group_size=d["group_size"],
        svd_rank=d["svd_rank"], svd_steps=8, codebook_steps=24, use_quantized_matmul=d["use_quantized_matmul"],
        re_quantize_for_matmul=d["re_quantize_for_matmul"], use_stochastic_rounding=False, use_hadamard=d["use_hadamard"],
        use_codebook=d["use_codebook"], layer_class_name=d["layer_class_name"])
    mod = get_sdnq_wrapper_class(layer, get_forward_func(d["layer_class_name"], d["quantized_matmul_dtype"], d["use_quantized_matmul"]))
    P = lambda x: torch.nn.Parameter(x.clone(), requires_grad=False)  # noqa: E731
    mod.weight, mod.scale = P(t["weight"]), P(t["scale"])
    mod.zero_point = P(t["zero_point"]) if "zero_point" in t else None
    mod.svd_up = mod.svd_down = None
    return mod if device is None else mod.to(device)


def output_padding(meta, t):
    """The output_padding the fixture's forward ran with (its own argument, or what `output_size=` resolves to)."""
    layer = float_layer(meta, t)
    if meta["output_size"] is None:
        return tuple(layer.output_padding)
    nd = meta["nd"]
    return tuple(layer._output_padding(t["x"], list(meta["output_size"]), list(layer.stride), list(layer.padding), list(layer.kernel_size), nd,
                                       list(layer.dilation)))


@functools.lru_cache(maxsize=None)
def ref64(name):
    """float64 F.conv_transposeNd of the fixture's reference-dequantized weight, input and bias, on the CPU."""
    meta, t = load(name)
    kw = layer_kwargs(meta)
    bias = t["bias"].double() if "bias" in t else None
    return FUNC[meta["nd"]](t["x"].double(), t["w_deq"].double(), bias, kw.get("stride", 1), kw.get("padding", 0), output_padding(meta, t),
                            kw.get("groups", 1), kw.get("dilation", 1))


def operand_layout(w_deq, groups):
    """[C_in, C_out / groups, *kernel] -> the float GEMM's operand [groups, P, C_in / groups] (sdnq_hip_dequant_convt's output)."""
    c_in = w_deq.shape[0]
    return w_deq.reshape(groups, c_in // groups, -1).transpose(1, 2).contiguous()


def bits(x):
    x = x.detach().cpu().contiguous()
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])
