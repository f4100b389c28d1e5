"""Dynamic quantization (use_dynamic_quantization=True) on the host: the per-layer dtype search against the reference's fixtures
(tests/golden/dyn_*, written by make_golden_dynamic.py), the config, save / load of a mixed-dtype model, and the C-ABI validation
of the fused loss entry point (sdnq_hip_dequant_loss) -- no GPU needed."""
import ctypes
import glob
import json
import os
import zlib

import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib
from sdnq_amd import quantizer as Q
from sdnq_amd.common import weights_dtype_order


_VIEW = {"bf16": torch.bfloat16, "f16": torch.float16, "fp8e4m3": torch.float8_e4m3fn, "fp8e5m2": torch.float8_e5m2, "bool": torch.bool}


def from_np(a, tag):
    """fixture array + dtype tag (make_golden.to_np) -> tensor; 16-bit floats / fp8 / bool are stored as raw bits"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(_VIEW[tag]) if tag in _VIEW else t


def to_np(t):
    """tensor -> (contiguous bytes as ndarray, dtype tag) in the fixture convention"""
    t = t.detach().cpu().contiguous()
    tag = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float8_e4m3fn: "fp8e4m3", torch.float8_e5m2: "fp8e5m2",
           torch.bool: "bool", torch.uint16: "u16"}.get(t.dtype, str(t.dtype).replace("torch.", ""))
    if tag in ("bf16", "f16"):
        return t.view(torch.uint16).numpy(), tag
    if tag in ("fp8e4m3", "fp8e5m2", "bool"):
        return t.view(torch.uint8).numpy(), tag
    return t.numpy(), tag


HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = sorted(os.path.basename(p)[4:-5] for p in glob.glob(os.path.join(GOLDEN, "dyn_*.json")))
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def load_fixture(name):
    with open(os.path.join(GOLDEN, f"dyn_{name}.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, f"dyn_{name}.npz"))


def float_model(meta, z, device="cpu"):
    model = torch.nn.Module()
    for lname, (kind, shape) in meta["geometry"].items():
        w = from_np(z[f"{lname}.w_float"], meta["tensors"][f"{lname}.w_float"]["dtype"])
        if kind == "linear":
            layer = torch.nn.Linear(shape[0], shape[1], bias=False)
        elif kind == "conv":
            layer = torch.nn.Conv2d(shape[0], shape[1], shape[2], padding=1, bias=False)
        else:
            layer = torch.nn.Embedding(*shape)
        layer = layer.to(w.dtype)
        with torch.no_grad():
            layer.weight.copy_(w)
        setattr(model, lname, layer.to(device))
    return model


def config(meta):
    cfg = dict(meta["cfg"])
    cfg.setdefault("minimum_allowed_numel", 4096)
    return Q.SDNQConfig(use_dynamic_quantization=True, **cfg)


def run_search(meta, z, device="cpu"):
    """-> (quantized model, config after the call, [(dtype, mse)] in evaluation order)"""
    trace = []
    real = Q._candidate_mse

    def spy(dq, data, original, ref):
        out = real(dq, data, original, ref)
        trace.append((dq.weights_dtype, float(out)))
        return out

    Q._candidate_mse = spy
    try:
        torch.manual_seed(zlib.crc32(meta["name"].encode()))  # the generator's seed: the SVD draws the same random projections
        model, cfg = Q.apply_sdnq_to_module(float_model(meta, z, device), config(meta))
    finally:
        Q._candidate_mse = real
    return model, cfg, trace


def check_against_fixture(meta, z, model, cfg, trace, rel):
    assert json.loads(json.dumps(dict(modules_dtype_dict=cfg.modules_dtype_dict, modules_to_not_use_matmul=cfg.modules_to_not_use_matmul,
                                      modules_to_not_convert=cfg.modules_to_not_convert))) == meta["lists"]
    want = [(d, m) for info in meta["layers"].values() for d, m in zip(info["candidates"], info["mse"])]
    assert [d for d, _ in trace] == [d for d, _ in want]
    for (d, got), (_, ref) in zip(trace, want):
        assert got == pytest.approx(ref, rel=rel, abs=1e-30), d
    for lname, info in meta["layers"].items():
        layer = getattr(model, lname)
        dq = getattr(layer, "sdnq_dequantizer", None)
        assert (dq.weights_dtype if dq is not None else "float") == info["chosen"], lname
        if dq is not None:
            for k in ("use_quantized_matmul", "re_quantize_for_matmul", "group_size", "hadamard_group_size", "use_hadamard",
                      "quantized_matmul_dtype", "quantized_weight_shape", "result_shape"):
                got = getattr(dq, k)
                got = list(got) if isinstance(got, torch.Size) else got
                assert got == info["deq"][k], (lname, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_search_matches_reference(name):
    meta, z = load_fixture(name)
    model, cfg, trace = run_search(meta, z)
    check_against_fixture(meta, z, model, cfg, trace, rel=1e-6)
    svd = bool(meta["cfg"].get("use_svd"))
    for lname, info in meta["layers"].items():
        layer = getattr(model, lname)
        for k in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
            key = f"{lname}.{k}"
            t = getattr(layer, k, None) if info["chosen"] != "float" else None
            if key not in z.files:
                assert t is None, key
                continue
            spec = meta["tensors"][key]
            assert list(t.shape) == spec["shape"] and to_np(t)[1] == spec["dtype"], key
            if svd:
                assert list(t.stride()) == spec["stride"], key  # random factors: the layout is the contract (as test_codebook_host)
            else:
                assert to_np(t)[0].tobytes() == z[key].tobytes(), key
        if info["chosen"] == "float":
            assert not hasattr(layer, "sdnq_dequantizer") and layer.weight.dtype == TORCH_DT[meta["dtype"]]


def test_fixture_coverage():
    """The fixtures cover what the search does: acceptance at the first candidate, integer and eXmY float walks, exhaustion,
    the quantized-matmul exclusion past 8 bits, Hadamard, SVD, codebook, conv, embedding, per-module threshold, mixed models."""
    metas = [load_fixture(n)[0] for n in FIXTURES]
    infos = [i for m in metas for i in m["layers"].values()]
    assert any(len(i["candidates"]) == 1 and i["chosen"] == i["candidates"][0] for i in infos)
    assert any(i["chosen"] == "float" for i in infos)
    assert any(i["chosen"].startswith("float") and i["chosen"] != "float" for i in infos)
    assert any(m["lists"]["modules_to_not_use_matmul"] for m in metas)
    for key in ("use_hadamard", "use_svd", "use_codebook", "quant_conv", "quant_embedding", "modules_quant_config"):
        assert any(m["cfg"].get(key) for m in metas), key
    assert any(len({i["chosen"] for i in m["layers"].values()}) >= 3 for m in metas)


def test_weights_dtype_order_matches_fixture_walks():
    """Every recorded walk is a run of consecutive entries of weights_dtype_order (codebook walks: its unsigned integers)."""
    for n in FIXTURES:
        meta, _ = load_fixture(n)
        for info in meta["layers"].values():
            c = info["candidates"]
            i = weights_dtype_order.index(c[0])
            order = weights_dtype_order[i:]
            if meta["cfg"].get("use_codebook"):
                order = [d for d in order if d.startswith("uint")]
            assert order[:len(c)] == c, (n, c)
    assert len(weights_dtype_order) == len(set(weights_dtype_order)) == 169


def test_config_accepts_dynamic_and_round_trips():
    cfg = Q.SDNQConfig(weights_dtype="uint4", use_dynamic_quantization=True, dynamic_loss_threshold=1e-3)
    d = cfg.to_dict()
    assert d["use_dynamic_quantization"] is True and d["dynamic_loss_threshold"] == 1e-3
    back = Q.SDNQConfig.from_dict(json.loads(json.dumps(d)))
    assert back.use_dynamic_quantization and back.dynamic_loss_threshold == 1e-3
    hf = pytest.importorskip("sdnq_amd.hf_quantizer")
    assert hf.SDNQConfig.from_dict(d).use_dynamic_quantization


def test_unknown_start_dtype_fails_as_reference():
    with pytest.raises(ValueError):
        Q.sdnq_quantize_layer_weight_dynamic(torch.randn(64, 64), "Linear", weights_dtype="float32")


def test_wide_codebook_search_raises_naming_the_layer():
    w = torch.randn(64, 256)
    with pytest.raises(NotImplementedError, match="blocks.0.weight"):
        Q.sdnq_quantize_layer_weight_dynamic(w, "Linear", weights_dtype="uint7", use_codebook=True, dynamic_loss_threshold=0.0,
                                             param_name="blocks.0.weight")


def test_default_threshold_and_plain_return():
    w = torch.randn(64, 256)
    out = Q.sdnq_quantize_layer_weight_dynamic(w, "Linear", weights_dtype="int8")  # 10 ** -4: int8 passes at once
    dq, data = out
    assert dq.weights_dtype == "int8" and data["weight"].dtype == torch.int8
    assert Q.sdnq_quantize_layer_weight_dynamic(w[:32, :64], "Linear", weights_dtype="uint15", dynamic_loss_threshold=0.0) is None


def test_module_override_switches_search_per_layer():
    torch.manual_seed(1)
    model = torch.nn.Module()
    model.a = torch.nn.Linear(256, 64, bias=False)
    model.b = torch.nn.Linear(256, 64, bias=False)
    cfg = Q.SDNQConfig(weights_dtype="int2", minimum_allowed_numel=4096, modules_quant_config={"b": {"use_dynamic_quantization": True}})
    model, cfg = Q.apply_sdnq_to_module(model, cfg)
    assert model.a.sdnq_dequantizer.weights_dtype == "int2"
    assert model.b.sdnq_dequantizer.weights_dtype != "int2" and cfg.modules_dtype_dict


def test_pre_quantized_never_searches(monkeypatch):
    calls = []
    monkeypatch.setattr(Q, "sdnq_quantize_layer_weight_dynamic", lambda *a, **k: calls.append(1))
    with torch.device("meta"):
        model = torch.nn.Module()
        model.a = torch.nn.Linear(256, 64, bias=False)
    cfg = Q.SDNQConfig(weights_dtype="int4", use_dynamic_quantization=True, modules_dtype_dict={"int8": ["a.weight"]})
    model = Q.sdnq_post_load_quant(model, quantization_config=cfg, pre_quantized=True)
    assert not calls and model.a.sdnq_dequantizer.weights_dtype == "int8"


def test_mixed_dtype_save_load_round_trip(tmp_path):
    """A searched model saves with its mixed modules_dtype_dict and loads back layer by layer, byte for byte."""
    meta, z = load_fixture("model_mixed")
    model, cfg, _ = run_search(meta, z)
    chosen = {n: getattr(model, n).sdnq_dequantizer.weights_dtype for n in meta["layers"]}
    assert len(set(chosen.values())) >= 3
    sdnq_amd.save_sdnq_model(model, str(tmp_path), sdnq_config=cfg)
    loaded = sdnq_amd.load_sdnq_model(str(tmp_path), model=float_model(meta, z, "meta"), device="cpu")
    for n, d in chosen.items():
        a, b = getattr(model, n), getattr(loaded, n)
        assert b.sdnq_dequantizer.weights_dtype == d
        assert b.sdnq_dequantizer.use_quantized_matmul == a.sdnq_dequantizer.use_quantized_matmul
    want, got = model.state_dict(), loaded.state_dict()
    assert sorted(want) == sorted(got)
    for k in want:
        assert torch.equal(want[k].contiguous().view(torch.uint8), got[k].contiguous().view(torch.uint8)), k


def test_dequant_loss_abi_validation_without_gpu():
    lib = _lib.load()
    assert lib.sdnq_hip_dequant_loss_workspace_bytes(0, 64) == -3
    assert lib.sdnq_hip_dequant_loss_workspace_bytes(4, 64) == 8
    assert lib.sdnq_hip_dequant_loss_workspace_bytes(1 << 20, 4096) == 2048 * 8
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    w = _lib.SdnqWeight(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=16, k=64, group_size=64, svd_rank=0,
                        svd_dtype=0, storage=0, kind=0, bits=4, exponent=0, mantissa=0, native_float=0)
    f = lib.sdnq_hip_dequant_loss
    assert f(ctypes.byref(w), 0, None, 0, 64, p, p, 64, None) == -1         # ref NULL
    assert f(ctypes.byref(w), 0, p, 0, 64, None, p, 64, None) == -1         # sum_out NULL
    assert f(ctypes.byref(w), 0, p, 0, 64, p, None, 64, None) == -1         # workspace NULL
    assert f(ctypes.byref(w), 0, p, 3, 64, p, p, 64, None) == -2            # ref dtype
    assert f(ctypes.byref(w), 0, p, 0, 32, p, p, 64, None) == -3            # ld_ref < K
    assert f(ctypes.byref(w), 48, p, 0, 64, p, p, 64, None) == -3           # Hadamard group not a power of two
    assert f(ctypes.byref(w), 1024, p, 0, 64, p, p, 64, None) == -3         # Hadamard group > 512
    assert f(ctypes.byref(w), 0, p + 4, 0, 64, p, p, 64, None) == -4        # ref misaligned
    assert f(ctypes.byref(w), 0, p, 1, 68, p, p, 64, None) == -4            # bf16 row stride not 16-byte aligned
    assert f(ctypes.byref(w), 0, p, 0, 64, p + 4, p, 64, None) == -4        # sum_out misaligned
    assert f(ctypes.byref(w), 0, p, 0, 64, p, p, 0, None) == -8             # workspace too small
    w.group_size = 48
    assert f(ctypes.byref(w), 0, p, 0, 64, p, p, 64, None) == -3            # K % group
