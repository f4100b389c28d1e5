#!/usr/bin/env python3
"""Capture golden vectors of quantized EMBEDDING layers from the REAL reference (Disty0/sdnq @ /root/reference).

Runs ONLY in the build container, like make_golden.py (same environment switches, same stand-in ``diffusers``, whose helpers
it imports): the reference's ``sdnq_quantize_layer`` quantizes a float ``nn.Embedding`` (or transformers'
``Gemma4TextScaledWordEmbedding``) with ``quant_embedding=True`` on CPU, its eager ``quantized_embedding_forward`` gathers the
rows of a few id tensors, and ``emb_<case>.npz / .json`` receive the float table, the stored tensors, the ids, the outputs and
the dequantizer record.  The fixtures are DATA only: no reference source is stored.

Usage:  python tests/golden/make_golden_embedding.py [<case name> ...]
        python tests/golden/make_golden_embedding.py --verify        # stored tensors -> reference layer -> forward == stored y
        python tests/golden/make_golden_embedding.py --regen-check   # regenerate into a temp dir, compare with the tracked files

Every case is self-seeded (`torch.manual_seed(crc32(name))` before quantizing: the SVD cases draw from the global generator).
"""
import json
import math
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (environment switches, stand-in diffusers, the reference on sys.path, to_np / from_np / deq_fields)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdnq import SDNQConfig, sdnq_quantize_layer  # noqa: E402  (the reference)

OUT_DIR = HERE  # --regen-check points this at a temp dir

# V rows of D columns; ids of shapes [1], [3, 7], [2, 1, 5] in int64 / int32 / int64, with repeats and the ids 0 and V-1
CASES = [
    dict(name="int8_rowwise_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int8", group_size=-1)),
    dict(name="int4_g32_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int4", group_size=32)),
    dict(name="uint4_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="uint4")),
    dict(name="int6_g128_f16", V=160, D=256, dtype="f16", cfg=dict(weights_dtype="int6", group_size=128)),
    dict(name="fp8_e4m3fn_f32", V=160, D=256, dtype="f32", cfg=dict(weights_dtype="float8_e4m3fn")),
    dict(name="fp4_e2m1fn_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="float4_e2m1fn")),
    dict(name="int8_had256_bf16", V=160, D=512, dtype="bf16", cfg=dict(weights_dtype="int8", use_hadamard=True, hadamard_group_size=256)),
    dict(name="int4_had64_f16", V=160, D=256, dtype="f16", cfg=dict(weights_dtype="int4", use_hadamard=True, hadamard_group_size=64)),
    dict(name="int4_svd_r8_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int4", use_svd=True, svd_rank=8)),
    dict(name="uint4_svd_r8_f32", V=160, D=256, dtype="f32", cfg=dict(weights_dtype="uint4", use_svd=True, svd_rank=8)),
    dict(name="int8_svd_r8_rowwise_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int8", group_size=-1, use_svd=True, svd_rank=8)),
    dict(name="int4_lpscale_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int4", dequantize_fp32=False)),
    dict(name="uint8_lpscale_f16", V=160, D=256, dtype="f16", cfg=dict(weights_dtype="uint8", group_size=-1, dequantize_fp32=False)),
    dict(name="gemma4_int8_scaled_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int8"), embed_scale=math.sqrt(3840),
         cls="Gemma4TextScaledWordEmbedding"),
    dict(name="gemma4_int4_had128_scaled_bf16", V=160, D=256, dtype="bf16", cfg=dict(weights_dtype="int4", use_hadamard=True, hadamard_group_size=128),
         embed_scale=math.sqrt(3840), cls="Gemma4TextScaledWordEmbedding"),
]
IDS_SHAPES = [(1,), (3, 7), (2, 1, 5)]
IDS_DTYPES = [torch.int64, torch.int32, torch.int64]


def make_embedding(case):
    """The float table of a case (seeded by its name) inside the layer class the case names."""
    V, D, dtype = case["V"], case["D"], G.TORCH_DT[case["dtype"]]
    g = torch.Generator().manual_seed(zlib.crc32(case["name"].encode()))
    w = torch.randn(V, D, generator=g) * 0.02
    cols = torch.randperm(D, generator=g)[: max(1, D // 64)]
    w[:, cols] *= 8.0
    if case.get("cls") == "Gemma4TextScaledWordEmbedding":
        from transformers.models.gemma4.modeling_gemma4 import Gemma4TextScaledWordEmbedding
        emb = Gemma4TextScaledWordEmbedding(V, D, padding_idx=0, embed_scale=case["embed_scale"])
    else:
        emb = torch.nn.Embedding(V, D)
    with torch.no_grad():
        emb.weight.copy_(w)
    return emb.to(dtype)


def make_ids(case):
    V = case["V"]
    g = torch.Generator().manual_seed(zlib.crc32(case["name"].encode()) + 1)
    out = []
    for shape, dt in zip(IDS_SHAPES, IDS_DTYPES):
        n = int(np.prod(shape))
        ids = torch.randint(0, V, (n,), generator=g)
        if n > 1:
            ids[0], ids[-1] = 0, V - 1
            ids[n // 2] = ids[1]  # a repeat
        else:
            ids[0] = V - 1
        out.append(ids.view(shape).to(dt))
    return out


def quantize(case):
    torch.manual_seed(zlib.crc32(case["name"].encode()))
    emb = make_embedding(case)
    layer, _ = sdnq_quantize_layer(emb, SDNQConfig(quant_embedding=True, **case["cfg"]))
    return emb, layer


def run_case(case):
    name = case["name"]
    w_float = make_embedding(case).weight.detach().clone()
    _, layer = quantize(case)
    arrays, tensors = {}, {}

    def put(key, t):
        a, tag = G.to_np(t)
        tensors[key] = {"shape": None if t is None else list(t.shape), "stride": None if t is None else list(t.stride()), "dtype": tag}
        if a is not None:
            arrays[key] = a

    put("w_float", w_float)
    for k in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
        put(k, getattr(layer, k, None))
    with torch.no_grad():
        for i, ids in enumerate(make_ids(case)):
            put(f"ids_{i}", ids)
            put(f"y_{i}", layer(ids))
    meta = dict(name=name, V=case["V"], D=case["D"], dtype=case["dtype"], cfg=case["cfg"], embed_scale=case.get("embed_scale"),
                cls=case.get("cls", "Embedding"), wrapper=type(layer).__name__, deq=G.deq_fields(layer.sdnq_dequantizer),
                state_dict_keys=sorted(layer.state_dict().keys()), n_ids=len(IDS_SHAPES), tensors=tensors)
    np.savez_compressed(os.path.join(OUT_DIR, f"emb_{name}.npz"), **arrays)
    with open(os.path.join(OUT_DIR, f"emb_{name}.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", name, type(layer).__name__, {k: v["shape"] for k, v in tensors.items() if not k.startswith(("ids", "y"))})


def verify():
    """Build the reference layer for each stored config, replace its tensors by the stored ones, run the reference forward on the
    stored ids and require the stored outputs bit for bit (provenance that does not depend on regenerating the SVD factors)."""
    bad = 0
    for case in CASES:
        name = case["name"]
        z = np.load(os.path.join(HERE, f"emb_{name}.npz"))
        with open(os.path.join(HERE, f"emb_{name}.json")) as f:
            meta = json.load(f)
        _, layer = quantize(case)
        assert G.deq_fields(layer.sdnq_dequantizer) == meta["deq"], name
        for k in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
            info = meta["tensors"][k]
            if info["shape"] is None:
                assert getattr(layer, k, None) is None, (name, k)
                continue
            t = G.from_np(z[k], info["dtype"])
            assert list(getattr(layer, k).shape) == info["shape"], (name, k)
            if list(t.stride()) != info["stride"]:  # stored as contiguous logical values: the reference's strides pick its BLAS path
                t = torch.empty_strided(tuple(t.shape), tuple(info["stride"]), dtype=t.dtype).copy_(t)
            setattr(layer, k, torch.nn.Parameter(t, requires_grad=False))
        with torch.no_grad():
            for i in range(meta["n_ids"]):
                ids = G.from_np(z[f"ids_{i}"], meta["tensors"][f"ids_{i}"]["dtype"])
                ya, _ = G.to_np(layer(ids))
                ok = np.array_equal(ya, z[f"y_{i}"])
                bad += not ok
                print("verify", name, i, "OK" if ok else f"MISMATCH {(ya != z[f'y_{i}']).sum()} elements")
    print("verify done, mismatching outputs:", bad)
    return bad


def regen_check():
    """Regenerate every fixture into a temp dir and compare array by array with the tracked files."""
    import tempfile
    global OUT_DIR
    OUT_DIR = tempfile.mkdtemp(prefix="sdnq_golden_emb_")
    generate(None)
    bad = 0
    for fn in sorted(os.listdir(OUT_DIR)):
        a, b = os.path.join(OUT_DIR, fn), os.path.join(HERE, fn)
        if not os.path.exists(b):
            print("regen-check: not tracked:", fn)
            bad += 1
        elif fn.endswith(".npz"):
            za, zb = np.load(a), np.load(b)
            same = sorted(za.files) == sorted(zb.files) and all(
                za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes() for k in za.files)
            bad += not same
            print("regen-check", fn, "identical" if same else "DIFFERS")
        else:
            same = open(a).read() == open(b).read()
            bad += not same
            print("regen-check", fn, "identical" if same else "DIFFERS")
    print("regen-check done, differing files:", bad, "(temp dir", OUT_DIR + ")")
    return bad


def generate(only):
    for c in CASES:
        if only is None or c["name"] in only:
            run_case(c)


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--verify" in sys.argv[1:]:
        sys.exit(1 if verify() else 0)
    if "--regen-check" in sys.argv[1:]:
        sys.exit(1 if regen_check() else 0)
    generate(sys.argv[1:] or None)
