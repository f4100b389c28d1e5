"""Quantized embeddings (SDNQConfig(quant_embedding=True)) on the host: the quantizer reproduces the reference's stored tensors
(tests/golden/emb_*, written by make_golden_embedding.py), the layer record, wrapper class and state_dict keys match, the forward
dispatch / support predicate / C ABI are in place, and checkpoints round-trip.  No GPU needed."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib
from sdnq_amd.forward import get_forward_func
from sdnq_amd.support import unsupported_reason

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
VIEW = {"bf16": torch.bfloat16, "f16": torch.float16, "fp8e4m3": torch.float8_e4m3fn}
REC = ["weights_dtype", "quantized_matmul_dtype", "hadamard_group_size", "group_size", "svd_rank", "use_quantized_matmul",
       "re_quantize_for_matmul", "use_hadamard", "use_codebook", "is_packed", "is_unsigned", "is_integer", "is_integer_matmul",
       "layer_class_name"]


def emb_case_names():
    return sorted(os.path.basename(p)[4:-5] for p in glob.glob(os.path.join(GOLDEN, "emb_*.json")))


def load_case(name):
    meta = json.load(open(os.path.join(GOLDEN, f"emb_{name}.json")))
    return meta, np.load(os.path.join(GOLDEN, f"emb_{name}.npz"))


def stored(z, meta, key):
    tag = meta["tensors"][key]["dtype"]
    if tag == "none":
        return None
    t = torch.from_numpy(np.ascontiguousarray(z[key]))
    return t.view(VIEW[tag]) if tag in VIEW else t


def float_layer(meta, z):
    """The case's float table in the layer class it was quantized from."""
    V, D = meta["V"], meta["D"]
    if meta["cls"] == "Gemma4TextScaledWordEmbedding":
        from transformers.models.gemma4.modeling_gemma4 import Gemma4TextScaledWordEmbedding
        emb = Gemma4TextScaledWordEmbedding(V, D, padding_idx=0, embed_scale=meta["embed_scale"])
    else:
        emb = torch.nn.Embedding(V, D)
    emb = emb.to(TORCH_DT[meta["dtype"]])
    with torch.no_grad():
        emb.weight.copy_(stored(z, meta, "w_float"))
    return emb


def quantize_case(meta, z, device="cpu"):
    emb = float_layer(meta, z).to(device)
    layer, cfg = sdnq_amd.sdnq_quantize_layer(emb, sdnq_amd.SDNQConfig(quant_embedding=True, **meta["cfg"]))
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
        assert got is not None and list(got.shape) == list(want.shape) and got.dtype == want.dtype, (key, got, want.shape)
        if svd:  # the factors come from a random low-rank solver: layout and shapes only
            continue
        got = got.detach().cpu().contiguous()
        assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)), f"{meta['name']}: {key} differs"


def test_quant_embedding_config_is_accepted():
    cfg = sdnq_amd.SDNQConfig(quant_embedding=True)
    assert cfg.quant_embedding and sdnq_amd.SDNQConfig.from_dict(cfg.to_dict()).quant_embedding


def test_fixtures_cover_the_issue_matrix():
    names = emb_case_names()
    assert len(names) >= 12
    metas = [load_case(n)[0] for n in names]
    assert any(m["embed_scale"] for m in metas) and any(m["cfg"].get("use_svd") for m in metas)
    assert any(m["cfg"].get("use_hadamard") for m in metas) and any(m["cfg"].get("dequantize_fp32") is False for m in metas)


@pytest.mark.parametrize("name", emb_case_names())
def test_host_quantizer_reproduces_reference_embedding(name):
    meta, z = load_case(name)
    torch.manual_seed(0)
    layer = quantize_case(meta, z)
    assert type(layer).__name__ == meta["wrapper"] == "SDNQEmbedding"
    assert isinstance(layer, sdnq_amd.layers.SDNQEmbedding) and isinstance(layer, torch.nn.Embedding)
    assert record(layer.sdnq_dequantizer) == meta["deq"]
    assert sorted(layer.state_dict().keys()) == meta["state_dict_keys"]
    check_stored_tensors(layer, meta, z)
    assert layer.forward_func is sdnq_amd.embedding.quantized_embedding_forward
    assert unsupported_reason(layer) is None
    if meta["embed_scale"]:
        assert layer.scalar_embed_scale == pytest.approx(math.sqrt(3840))


def test_forward_dispatch_and_support_predicate():
    for cls in ("Embedding", "SDNQEmbedding", "Gemma4TextScaledWordEmbedding"):
        assert get_forward_func(cls, "int8", False) is sdnq_amd.embedding.quantized_embedding_forward
    layer, _ = sdnq_amd.sdnq_quantize_layer(torch.nn.Embedding(64, 40), sdnq_amd.SDNQConfig(quant_embedding=True, weights_dtype="int8"))
    assert "multiple of 16" in unsupported_reason(layer)
    layer, _ = sdnq_amd.sdnq_quantize_layer(torch.nn.Embedding(64, 64), sdnq_amd.SDNQConfig(quant_embedding=True, weights_dtype="int4"))
    assert unsupported_reason(layer) is None
    layer.sdnq_dequantizer.use_codebook = True
    assert "codebook" in unsupported_reason(layer)


def test_cpu_forward_raises():
    layer, _ = sdnq_amd.sdnq_quantize_layer(torch.nn.Embedding(64, 64), sdnq_amd.SDNQConfig(quant_embedding=True, weights_dtype="int8"))
    with pytest.raises(_lib.SdnqHipError):
        layer(torch.tensor([1, 2]))


def test_embeddings_are_listed_without_quant_embedding():
    model = torch.nn.Sequential(torch.nn.Embedding(256, 128), torch.nn.Linear(128, 128))
    model, cfg = sdnq_amd.apply_sdnq_to_module(model, sdnq_amd.SDNQConfig(weights_dtype="int8"))
    assert type(model[0]) is torch.nn.Embedding and "0.weight" in cfg.modules_to_not_convert
    model = torch.nn.Sequential(torch.nn.Embedding(256, 128), torch.nn.Linear(128, 128))
    model, cfg = sdnq_amd.apply_sdnq_to_module(model, sdnq_amd.SDNQConfig(weights_dtype="int8", quant_embedding=True))
    assert isinstance(model[0], sdnq_amd.layers.SDNQEmbedding) and "0.weight" not in cfg.modules_to_not_convert


def test_sdnq_layers_reexports_the_embedding_wrapper():
    import sdnq.layers
    assert sdnq.layers.SDNQEmbedding is sdnq_amd.layers.SDNQEmbedding


def test_embedding_export_and_argtypes():
    lib = _lib.load()
    assert "sdnq_hip_embedding" in _lib.EXPORTS
    cfn = getattr(lib, "_ctypes", lib).sdnq_hip_embedding  # ctypes declaration (the typed binding, when built, serves the same symbol)
    assert cfn.argtypes is not None and len(cfn.argtypes) == 10
    import ctypes
    buf = ctypes.create_string_buffer(4096)  # validation runs before any launch: no device memory is touched
    p = ctypes.addressof(buf)
    p += (-p) % 16
    w = _lib.SdnqWeight(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=16, k=64, group_size=64, svd_rank=0,
                        svd_dtype=0, storage=2, kind=0, bits=8, exponent=0, mantissa=0, native_float=0, positions=1, scale_dtype=0)
    assert lib.sdnq_hip_embedding(ctypes.addressof(w), 0, p, 7, 4, 0, 0.0, p, 1, None) == -2        # ids dtype
    assert lib.sdnq_hip_embedding(ctypes.addressof(w), 48, p, 1, 4, 0, 0.0, p, 1, None) == -3       # Hadamard group not a power of two
    assert lib.sdnq_hip_embedding(ctypes.addressof(w), 0, p, 1, 4, 0, 0.0, p + 2, 1, None) == -4    # output alignment
    assert lib.sdnq_hip_embedding(ctypes.addressof(w), 0, None, 1, 4, 0, 0.0, p, 1, None) == -1     # ids NULL
    assert lib.sdnq_hip_embedding(ctypes.addressof(w), 0, p, 1, 0, 0, 0.0, p, 1, None) == 0         # nothing to gather: no launch
    w.k = 40
    assert lib.sdnq_hip_embedding(ctypes.addressof(w), 0, p, 1, 4, 0, 0.0, p, 1, None) == -3        # D % 16


class TinyEmbNet(torch.nn.Module):
    def __init__(self, vocab=256, dim=128):
        super().__init__()
        self.embed_tokens = torch.nn.Embedding(vocab, dim)
        self.proj = torch.nn.Linear(dim, dim)


def test_save_and_load_round_trip(tmp_path):
    torch.manual_seed(0)
    model = TinyEmbNet().to(torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="uint4", quant_embedding=True, use_svd=True, svd_rank=4)
    model = sdnq_amd.sdnq_post_load_quant(model, quantization_config=cfg)
    assert isinstance(model.embed_tokens, sdnq_amd.layers.SDNQEmbedding)
    assert {"embed_tokens.weight", "embed_tokens.scale", "embed_tokens.zero_point", "embed_tokens.svd_up",
            "embed_tokens.svd_down"} <= set(model.state_dict())
    sdnq_amd.save_sdnq_model(model, str(tmp_path))
    with torch.device("meta"):
        skeleton = TinyEmbNet().to(torch.bfloat16)
    loaded = sdnq_amd.load_sdnq_model(str(tmp_path), model=skeleton, device="cpu")
    assert isinstance(loaded.embed_tokens, sdnq_amd.layers.SDNQEmbedding)
    assert loaded.embed_tokens.forward_func is sdnq_amd.embedding.quantized_embedding_forward
    assert record(loaded.embed_tokens.sdnq_dequantizer) == record(model.embed_tokens.sdnq_dequantizer)
    want, got = model.state_dict(), loaded.state_dict()
    assert sorted(want) == sorted(got)
    for k in want:
        assert torch.equal(want[k].contiguous().view(torch.uint8), got[k].contiguous().view(torch.uint8)), k
    # dtype / dequantize_fp32 options reach the embedding: 16-bit scales in the result dtype
    sdnq_amd.apply_sdnq_options_to_model(loaded, dequantize_fp32=False)
    assert loaded.embed_tokens.scale.dtype == torch.bfloat16 and unsupported_reason(loaded.embed_tokens) is None


def test_sharding_slices_the_linears_and_leaves_the_embedding_whole():
    """Column sharding (sdnq_amd.parallel) is built for quantized Linear layers: a model with an SDNQEmbedding shards its Linears and the
    embedding stays one replicated table -- shard_quantized_module refuses it instead of slicing it, and its tensors are untouched."""
    from sdnq_amd.parallel import shard_bounds, shard_quantized_module
    torch.manual_seed(0)
    model = TinyEmbNet().to(torch.bfloat16)
    model = sdnq_amd.sdnq_post_load_quant(model, quantization_config=sdnq_amd.SDNQConfig(weights_dtype="int4", quant_embedding=True))
    before = {k: v.clone() for k, v in model.embed_tokens.state_dict().items()}
    world, n = 2, model.proj.sdnq_dequantizer.out_features
    shards, replicated = {}, []
    for name, mod in model.named_modules():
        if getattr(mod, "sdnq_dequantizer", None) is None:
            continue
        try:
            shards[name] = [shard_quantized_module(mod, *shard_bounds(n, r, world)) for r in range(world)]
        except NotImplementedError:
            replicated.append(name)
    assert list(shards) == ["proj"] and replicated == ["embed_tokens"]
    assert torch.equal(torch.cat([p.weight for p in shards["proj"]], 0), model.proj.weight)
    for k, v in model.embed_tokens.state_dict().items():
        assert torch.equal(v, before[k]), k
