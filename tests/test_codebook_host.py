"""Codebook quantization (SDNQConfig(use_codebook=True)) on the host: the quantizer reproduces the reference's stored codes and level
tables byte for byte (tests/golden/cb_*, written by make_golden_codebook.py), the group policy, layer record and support predicate
follow the reference, checkpoints round-trip, and the C ABI validates the new kind and entry point.  No GPU needed."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib
from sdnq_amd.quantizer import _pick_group_size
from sdnq_amd.support import unsupported_reason

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
VIEW = {"bf16": torch.bfloat16, "f16": torch.float16, "fp8e4m3": torch.float8_e4m3fn, "bool": torch.bool}
REC = ["weights_dtype", "quantized_matmul_dtype", "hadamard_group_size", "group_size", "svd_rank", "use_quantized_matmul",
       "re_quantize_for_matmul", "use_hadamard", "use_codebook", "is_packed", "is_unsigned", "is_integer", "is_integer_matmul",
       "layer_class_name"]


def cb_case_names():
    return sorted(os.path.basename(p)[3:-5] for p in glob.glob(os.path.join(GOLDEN, "cb_*.json")))


def load_case(name):
    meta = json.load(open(os.path.join(GOLDEN, f"cb_{name}.json")))
    return meta, np.load(os.path.join(GOLDEN, f"cb_{name}.npz"))


def stored(z, meta, key):
    tag = meta["tensors"][key]["dtype"]
    if tag == "none":
        return None
    t = torch.from_numpy(np.ascontiguousarray(z[key]))
    return t.view(VIEW[tag]) if tag in VIEW else t


def float_layer(meta, z):
    """The case's float layer (Linear / Conv2d / Embedding) holding the stored float weight (and a zero bias where it has one)."""
    w = stored(z, meta, "w_float")
    g = meta["geometry"]
    if meta["kind"] == "linear":
        layer = torch.nn.Linear(g["K"], g["N"])
    elif meta["kind"] == "conv":
        layer = torch.nn.Conv2d(g["cin"], g["cout"], g["k"], padding=1)
    else:
        layer = torch.nn.Embedding(g["V"], g["D"])
    layer = layer.to(TORCH_DT[meta["dtype"]])
    with torch.no_grad():
        layer.weight.copy_(w)
        if getattr(layer, "bias", None) is not None and meta["tensors"]["bias"]["dtype"] != "none":
            layer.bias.copy_(stored(z, meta, "bias"))
    return layer


def config_of(meta):
    extra = {"conv": dict(quant_conv=True), "embedding": dict(quant_embedding=True)}.get(meta["kind"], {})
    return sdnq_amd.SDNQConfig(use_codebook=True, **extra, **meta["cfg"])


def quantize_case(meta, z, device="cpu"):
    layer, _ = sdnq_amd.sdnq_quantize_layer(float_layer(meta, z).to(device), config_of(meta))
    return layer


def record(dq):
    d = {k: getattr(dq, k) for k in REC}
    d["result_dtype"] = str(dq.result_dtype).replace("torch.", "")
    d["result_shape"] = list(dq.result_shape) if dq.result_shape is not None else None
    d["quantized_weight_shape"] = list(dq.quantized_weight_shape)
    d["original_shape"] = list(dq.original_shape)
    return d


def check_stored_tensors(layer, meta, z):
    svd = meta["cfg"].get("use_svd", False)
    for key in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
        want = stored(z, meta, key)
        got = getattr(layer, key, None)
        if want is None:
            assert got is None, key
            continue
        assert got is not None and list(got.shape) == list(want.shape), (key, None if got is None else got.shape, want.shape)
        if svd:  # the factors come from a random low-rank solver, and with them the residual the codebook is fitted to
            continue
        got = got.detach().cpu().contiguous()
        assert got.element_size() == want.element_size(), key
        assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)), f"{meta['name']}: {key} differs"


def test_fixtures_cover_the_issue_matrix():
    metas = [load_case(n)[0] for n in cb_case_names()]
    assert len(metas) >= 15
    dts = {m["cfg"]["weights_dtype"] for m in metas}
    assert {"uint1", "uint2", "uint3", "uint4", "uint8"} <= dts
    mms = {m["deq"]["quantized_matmul_dtype"] for m in metas if m["deq"]["use_quantized_matmul"]}
    assert {"int8", "uint8", "float8_e4m3fn"} <= mms
    assert any(not m["deq"]["use_quantized_matmul"] and m["kind"] == "linear" for m in metas)
    assert any(m["cfg"].get("use_svd") for m in metas) and any(m["cfg"].get("use_hadamard") for m in metas)
    assert any(m["cfg"].get("dequantize_fp32") is False for m in metas)
    assert {m["kind"] for m in metas} == {"linear", "conv", "embedding"}
    assert any(m["deq"]["group_size"] == -1 for m in metas) and any(m["deq"]["group_size"] > 0 for m in metas)


@pytest.mark.parametrize("name", cb_case_names())
def test_host_quantizer_reproduces_reference_codebook(name):
    """Codes (packed bytes), level table and dequantizer record of every cb_* fixture, byte for byte."""
    meta, z = load_case(name)
    torch.manual_seed(0)
    layer = quantize_case(meta, z)
    assert record(layer.sdnq_dequantizer) == meta["deq"]
    assert layer.sdnq_dequantizer.use_codebook and layer.sdnq_dequantizer.codebook_steps == meta["codebook_steps"]
    assert layer.forward_func.__name__ == meta["forward_func"]
    check_stored_tensors(layer, meta, z)
    assert unsupported_reason(layer) is None


def test_constant_and_midpoint_rows():
    """The ties fixture: a constant row keeps one occupied level, values on a midpoint take the lower level."""
    meta, z = load_case("lin_uint2_steps6_ties_int8mm_f32")
    layer = quantize_case(meta, z)
    levels = layer.scale.view(48, -1, 4)
    assert torch.all(levels[0] == 0.25)
    check_stored_tensors(layer, meta, z)


def test_codebook_config_round_trip_and_dtypes():
    cfg = sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True, codebook_steps=12)
    again = sdnq_amd.SDNQConfig.from_dict(json.loads(json.dumps(cfg.to_dict())))
    assert again.use_codebook and again.codebook_steps == 12 and again.weights_dtype == "uint4"
    for dt in ("uint1", "uint2", "uint3", "uint5", "uint7", "uint8"):
        assert sdnq_amd.SDNQConfig(weights_dtype=dt, use_codebook=True).use_codebook
    for dt in ("int8", "int4", "float8_e4m3fn"):
        with pytest.raises(NotImplementedError, match="only supported with unsigned integer dtypes"):
            sdnq_amd.SDNQConfig(weights_dtype=dt, use_codebook=True)
    with pytest.raises(NotImplementedError, match="codebook"):
        sdnq_amd.SDNQConfig(weights_dtype="uint16", use_codebook=True)


def test_codebook_steps_reach_the_quantizer():
    torch.manual_seed(3)
    lin = torch.nn.Linear(256, 64)
    a, _ = sdnq_amd.sdnq_quantize_layer(_copy(lin), sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True, codebook_steps=0))
    b, _ = sdnq_amd.sdnq_quantize_layer(_copy(lin), sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True))
    assert a.sdnq_dequantizer.codebook_steps == 0 and b.sdnq_dequantizer.codebook_steps == 24
    # zero steps: the evenly spaced initial levels
    lo, hi = lin.weight.detach().min(dim=1).values, lin.weight.detach().max(dim=1).values
    assert torch.equal(a.scale[:, 0], lo) and torch.allclose(a.scale[:, -1], hi)
    assert not torch.equal(a.scale, b.scale)


def _copy(lin):
    out = torch.nn.Linear(lin.in_features, lin.out_features)
    out.load_state_dict(lin.state_dict())
    return out


def test_group_policy():
    """The default group gets +3 in its power of two with use_codebook (the reference's quantizer.py:182-183)."""
    assert _pick_group_size(0, 4096, "uint4", True, False, False, codebook=True) == (512, 8)
    assert _pick_group_size(0, 4096, "uint4", True, True, False, codebook=True) == (1024, 4)
    assert _pick_group_size(0, 4096, "uint8", True, False, False, codebook=True) == (-1, 1)     # 8192 >= K: row-wise
    assert _pick_group_size(0, 16384, "uint8", True, False, False, codebook=True) == (8192, 2)
    assert _pick_group_size(0, 4096, "uint4", False, False, False, codebook=True) == (256, 16)  # embeddings / convs
    assert _pick_group_size(0, 4096, "uint4", True, False, False) == (64, 64)                  # unchanged without a codebook
    lin, _ = sdnq_amd.sdnq_quantize_layer(torch.nn.Linear(2048, 64), sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True,
                                                                                          use_quantized_matmul=True))
    dq = lin.sdnq_dequantizer
    assert dq.group_size == 512 and dq.re_quantize_for_matmul and dq.quantized_matmul_dtype == "int8"
    assert tuple(lin.scale.shape) == (64, 4, 16) and lin.zero_point is None
    u8, _ = sdnq_amd.sdnq_quantize_layer(torch.nn.Linear(512, 64), sdnq_amd.SDNQConfig(weights_dtype="uint8", use_codebook=True,
                                                                                        use_quantized_matmul=True))
    assert u8.sdnq_dequantizer.quantized_matmul_dtype == "uint8" and u8.sdnq_dequantizer.re_quantize_for_matmul
    assert tuple(u8.scale.shape) == (64, 256) and u8.weight.dtype == torch.uint8


def _layer(kind="linear", **cfg):
    torch.manual_seed(0)
    if kind == "conv":
        mod = torch.nn.Conv2d(64, 64, 3, padding=1)
        extra = dict(quant_conv=True)
    elif kind == "embedding":
        mod = torch.nn.Embedding(64, 128)
        extra = dict(quant_embedding=True)
    else:
        mod = torch.nn.Linear(256, 64)
        extra = {}
    layer, _ = sdnq_amd.sdnq_quantize_layer(mod, sdnq_amd.SDNQConfig(use_codebook=True, **extra, **cfg))
    return layer


def test_support_predicate_sentences():
    assert unsupported_reason(_layer(weights_dtype="uint4", use_quantized_matmul=True)) is None
    assert unsupported_reason(_layer(weights_dtype="uint8", use_quantized_matmul=True)) is None
    assert unsupported_reason(_layer(weights_dtype="uint2", use_quantized_matmul=True, quantized_matmul_dtype="float8_e4m3fn")) is None
    assert unsupported_reason(_layer("conv", weights_dtype="uint4", group_size=32, use_quantized_matmul_conv=True)) is None
    assert unsupported_reason(_layer("conv", weights_dtype="uint4")) is None
    assert unsupported_reason(_layer("embedding", weights_dtype="uint4", group_size=32)) is None
    # refused configurations: one sentence each, all naming the codebook
    lay = _layer(weights_dtype="uint4")
    lay.sdnq_dequantizer.weights_dtype = "int4"
    assert "codebook" in unsupported_reason(lay) and "unsigned" in unsupported_reason(lay)
    lay = _layer(weights_dtype="uint4")
    lay.sdnq_dequantizer.weights_dtype = "uint12"
    assert "codebook" in unsupported_reason(lay) and "8 bits" in unsupported_reason(lay)
    lay = _layer(weights_dtype="uint4")
    lay.sdnq_dequantizer.group_size = -2
    assert "codebook" in unsupported_reason(lay) and "tensorwise" in unsupported_reason(lay)
    conv = _layer("conv", weights_dtype="uint4", use_quantized_matmul_conv=True)
    assert conv.sdnq_dequantizer.group_size == -1 and conv.sdnq_dequantizer.use_quantized_matmul
    assert "codebook" in unsupported_reason(conv) and "ungrouped" in unsupported_reason(conv)
    lay = _layer(weights_dtype="uint4", use_quantized_matmul=True, quantized_matmul_dtype="float16")
    assert "codebook" in unsupported_reason(lay) and "float16" in unsupported_reason(lay)


def test_accelerate_leaves_no_codebook_layer_behind_on_cpu_models():
    """accelerate() judges codebook layers like any other: a built configuration is adopted (nothing skipped)."""
    model = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.GELU(), torch.nn.Linear(128, 64))
    model = sdnq_amd.sdnq_post_load_quant(model, quantization_config=sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True,
                                                                                         use_quantized_matmul=True,
                                                                                         minimum_allowed_numel=0))
    res = sdnq_amd.accelerate(model)
    assert res.accelerated == 2 and not res.skipped


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embed_tokens = torch.nn.Embedding(128, 128)
        self.proj = torch.nn.Linear(128, 256)
        self.conv = torch.nn.Conv2d(64, 64, 3, padding=1)


def test_save_and_load_round_trip(tmp_path):
    torch.manual_seed(0)
    model = TinyNet().to(torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True, quant_embedding=True, quant_conv=True, group_size=32,
                              use_quantized_matmul=True, use_quantized_matmul_conv=True, minimum_allowed_numel=0)
    model = sdnq_amd.sdnq_post_load_quant(model, quantization_config=cfg)
    assert all(m.sdnq_dequantizer.use_codebook for m in (model.embed_tokens, model.proj, model.conv))
    sdnq_amd.save_sdnq_model(model, str(tmp_path))
    with torch.device("meta"):
        skeleton = TinyNet().to(torch.bfloat16)
    loaded = sdnq_amd.load_sdnq_model(str(tmp_path), model=skeleton, device="cpu")
    for name in ("embed_tokens", "proj", "conv"):
        assert record(getattr(loaded, name).sdnq_dequantizer) == record(getattr(model, name).sdnq_dequantizer), name
        assert unsupported_reason(getattr(loaded, name)) is None
    want, got = model.state_dict(), loaded.state_dict()
    assert sorted(want) == sorted(got)
    for k in want:
        assert torch.equal(want[k].contiguous().view(torch.uint8), got[k].contiguous().view(torch.uint8)), k
    # dtype / dequantize_fp32 options reach codebook layers too: the level tables take the result dtype
    sdnq_amd.apply_sdnq_options_to_model(loaded, dequantize_fp32=False)
    assert loaded.proj.scale.dtype == torch.bfloat16 and unsupported_reason(loaded.proj) is None


def test_codebook_abi_validation():
    """The new kind and entry point validate before any launch (no device memory is touched)."""
    assert _lib.KIND_CODEBOOK == 4 and "sdnq_hip_quantize_codebook" in _lib.EXPORTS
    lib = _lib.load()
    cfn = getattr(lib, "_ctypes", lib)
    assert cfn.sdnq_hip_quantize_codebook.argtypes is not None and len(cfn.sdnq_hip_quantize_codebook.argtypes) == 6
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def w(**kw):
        d = dict(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=16, k=64, group_size=64, svd_rank=0, svd_dtype=0,
                 storage=0, kind=4, bits=4, exponent=0, mantissa=0, native_float=0, positions=1, scale_dtype=0)
        d.update(kw)
        return _lib.SdnqWeight(**d)

    q = cfn.sdnq_hip_quantize_codebook
    assert q(p, 0, 64, ctypes.byref(w(kind=1)), 24, None) == -2                 # not the codebook kind
    assert q(p, 0, 64, ctypes.byref(w(bits=9, storage=1)), 24, None) == -2      # wider than 8 bits
    assert q(p, 0, 64, ctypes.byref(w(bits=8, storage=0)), 24, None) == -2      # 8-bit codes are raw bytes
    assert q(p, 0, 64, ctypes.byref(w(zero_point=p)), 24, None) == -5           # a codebook has no zero point
    assert q(p, 0, 64, ctypes.byref(w(group_size=48)), 24, None) == -3          # group does not divide K
    assert q(p, 0, 32768, ctypes.byref(w(n=1, k=32768, group_size=32768)), 24, None) == -5  # slice longer than the kernel's LDS
    assert q(p, 0, 64, ctypes.byref(w()), -1, None) == -5                       # steps
    assert q(p, 5, 64, ctypes.byref(w()), 24, None) == -2                       # source dtype
    assert q(None, 0, 64, ctypes.byref(w()), 24, None) == -1
    assert q(p, 0, 64, ctypes.byref(w(weight=p + 2)), 24, None) == -4
    # the weight-side entry points accept the kind and validate its storage
    d = cfn.sdnq_hip_dequant
    assert d(ctypes.byref(w(bits=8, storage=0)), 0, p, 0, None) == -2
    assert d(ctypes.byref(w(zero_point=p)), 0, p, 0, None) == -5
    assert d(ctypes.byref(w(kind=5)), 0, p, 0, None) == -2
    assert cfn.sdnq_hip_unpack_mm(ctypes.byref(w()), 0, p, None) == -2        # codes are no matmul operand
