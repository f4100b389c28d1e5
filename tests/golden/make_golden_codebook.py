#!/usr/bin/env python3
"""Capture golden vectors of CODEBOOK-quantized layers (use_codebook=True) from the REAL reference (Disty0/sdnq @ /root/reference).

Runs ONLY in the build container, like make_golden.py (same environment switches, same stand-in ``diffusers``, whose helpers it
imports): the reference's ``sdnq_quantize_layer`` quantizes a float Linear / conv / embedding with ``use_codebook=True`` on CPU
(its Lloyd-Max quantizer), and ``cb_<case>.npz / .json`` receive the float weight, the stored tensors (packed codes, level
table), the reference's dequantized weight, its ``re_quantize_matmul`` outputs for quantized-matmul layers, inputs, forward
outputs and the dequantizer record.  The fixtures are DATA only: no reference source is stored.

Usage:  python tests/golden/make_golden_codebook.py [<case name> ...]
        python tests/golden/make_golden_codebook.py --verify        # stored tensors -> reference layer -> forward == stored y
        python tests/golden/make_golden_codebook.py --regen-check   # regenerate into a temp dir, compare with the tracked files

Every case is self-seeded (`torch.manual_seed(crc32(name))` before quantizing: the SVD case draws from the global generator).
"""
import json
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

# kind: linear (K, N, Ms), conv (cin, cout, k, groups-free Conv2d, input shapes), embedding (V, D, ids)
CASES = [
    dict(name="lin_uint4_g512_int8mm_bf16", kind="linear", K=1024, N=32, Ms=[8, 40], dtype="bf16",
         cfg=dict(weights_dtype="uint4", use_quantized_matmul=True)),
    dict(name="lin_uint4_g512_float_f16", kind="linear", K=1024, N=32, Ms=[4, 40], dtype="f16", cfg=dict(weights_dtype="uint4")),
    dict(name="lin_uint8_rowwise_uint8mm_bf16", kind="linear", K=512, N=32, Ms=[8, 40], dtype="bf16",
         cfg=dict(weights_dtype="uint8", use_quantized_matmul=True)),
    dict(name="lin_uint8_g128_int8mm_f16", kind="linear", K=512, N=32, Ms=[40], dtype="f16",
         cfg=dict(weights_dtype="uint8", group_size=128, use_quantized_matmul=True, quantized_matmul_dtype="int8")),
    dict(name="lin_uint2_g128_fp8mm_bf16", kind="linear", K=512, N=64, Ms=[40], dtype="bf16",
         cfg=dict(weights_dtype="uint2", group_size=128, use_quantized_matmul=True, quantized_matmul_dtype="float8_e4m3fn")),
    dict(name="lin_uint3_rowwise_float_f32", kind="linear", K=256, N=48, Ms=[4, 40], dtype="f32",
         cfg=dict(weights_dtype="uint3", group_size=-1)),
    dict(name="lin_uint1_g64_float_bf16", kind="linear", K=256, N=48, Ms=[40], dtype="bf16", cfg=dict(weights_dtype="uint1", group_size=64)),
    dict(name="lin_uint4_svd_r16_int8mm_bf16", kind="linear", K=1024, N=32, Ms=[8, 40], dtype="bf16",
         cfg=dict(weights_dtype="uint4", use_svd=True, svd_rank=16, use_quantized_matmul=True)),
    dict(name="lin_uint4_had128_int8mm_bf16", kind="linear", K=512, N=64, Ms=[8, 40], dtype="bf16",
         cfg=dict(weights_dtype="uint4", group_size=128, use_hadamard=True, hadamard_group_size=128, use_quantized_matmul=True)),
    dict(name="lin_uint4_lpscale_int8mm_bf16", kind="linear", K=1024, N=32, Ms=[8, 40], dtype="bf16",
         cfg=dict(weights_dtype="uint4", dequantize_fp32=False, use_quantized_matmul=True)),
    dict(name="lin_uint2_steps6_ties_int8mm_f32", kind="linear", K=256, N=48, Ms=[40], dtype="f32", ties=True,
         cfg=dict(weights_dtype="uint2", group_size=64, codebook_steps=6, use_quantized_matmul=True)),
    dict(name="conv_uint4_g32_int8mm_bf16", kind="conv", cin=64, cout=64, k=3, xs=[(2, 10, 10)], dtype="bf16",
         cfg=dict(weights_dtype="uint4", group_size=32, use_quantized_matmul_conv=True)),
    dict(name="conv_uint4_rowwise_float_f16", kind="conv", cin=32, cout=32, k=3, xs=[(2, 9, 9)], dtype="f16",
         cfg=dict(weights_dtype="uint4")),
    dict(name="emb_uint4_g64_bf16", kind="embedding", V=96, D=256, dtype="bf16", cfg=dict(weights_dtype="uint4", group_size=64)),
    dict(name="emb_uint8_rowwise_f32", kind="embedding", V=96, D=256, dtype="f32", cfg=dict(weights_dtype="uint8")),
]


def _ties(w):
    """Rows that exercise the degenerate cases: a constant row and rows of small integers, whose level midpoints the values hit
    exactly (such a value takes the lower level)."""
    w = w.clone()
    w[0] = 0.25
    k = w.shape[1]
    w[1] = (torch.arange(k) % 4).to(w.dtype)        # 0 1 2 3: with 4 levels every value sits on a level or a midpoint
    w[2] = (torch.arange(k) % 3).to(w.dtype)        # 0 1 2 into 4 levels
    w[3] = (torch.arange(k) % 5).to(w.dtype) * 0.5  # 0 .. 2 in halves
    return w


def make_layer(case):
    dtype = G.TORCH_DT[case["dtype"]]
    seed = zlib.crc32(case["name"].encode())
    if case["kind"] == "linear":
        lin = G.make_linear(case["K"], case["N"], seed=seed % 1000, dtype=torch.float32)
        if case.get("ties"):
            with torch.no_grad():
                lin.weight.copy_(_ties(lin.weight))
        return lin.to(dtype)
    g = torch.Generator().manual_seed(seed)
    if case["kind"] == "conv":
        conv = torch.nn.Conv2d(case["cin"], case["cout"], case["k"], padding=1)
        with torch.no_grad():
            w = torch.randn(conv.weight.shape, generator=g) * 0.05
            w[:, 3] *= 6.0
            conv.weight.copy_(w)
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.1)
        return conv.to(dtype)
    emb = torch.nn.Embedding(case["V"], case["D"])
    with torch.no_grad():
        w = torch.randn(case["V"], case["D"], generator=g) * 0.02
        w[:, torch.randperm(case["D"], generator=g)[:4]] *= 8.0
        emb.weight.copy_(w)
    return emb.to(dtype)


def make_inputs(case):
    dtype = G.TORCH_DT[case["dtype"]]
    seed = zlib.crc32(case["name"].encode())
    if case["kind"] == "linear":
        return [G.make_input(M, case["K"], seed=i, dtype=dtype) for i, M in enumerate(case["Ms"])]
    g = torch.Generator().manual_seed(seed + 1)
    if case["kind"] == "conv":
        out = []
        for shp in case["xs"]:
            x = torch.randn(shp[0], case["cin"], *shp[1:], generator=g)
            x[:, 1] *= 15.0
            out.append(x.to(dtype))
        return out
    ids = torch.randint(0, case["V"], (3, 7), generator=g)
    ids[0, 0], ids[-1, -1] = 0, case["V"] - 1
    return [ids, ids[1].to(torch.int32)]


def quantize(case):
    torch.manual_seed(zlib.crc32(case["name"].encode()))
    layer = make_layer(case)
    extra = {"conv": dict(quant_conv=True), "embedding": dict(quant_embedding=True)}.get(case["kind"], {})
    q, _ = sdnq_quantize_layer(layer, SDNQConfig(use_codebook=True, **extra, **case["cfg"]))
    return q


def run_case(case):
    name = case["name"]
    w_float = make_layer(case).weight.detach().clone()
    layer = quantize(case)
    dq = layer.sdnq_dequantizer
    arrays, tensors = {}, {}

    def put(key, t):
        a, tag = G.to_np(t)
        tensors[key] = {"shape": None if t is None else list(t.shape), "stride": None if t is None else list(t.stride()), "dtype": tag}
        if a is not None:
            arrays[key] = a

    put("w_float", w_float)
    for k in ("weight", "scale", "zero_point", "svd_up", "svd_down", "bias"):
        put(k, getattr(layer, k, None))
    with torch.no_grad():
        if case["kind"] != "embedding":
            put("w_dequant", dq(layer.weight, layer.scale, zero_point=layer.zero_point, svd_up=layer.svd_up, svd_down=layer.svd_down,
                                skip_quantized_matmul=dq.use_quantized_matmul))
        if dq.use_quantized_matmul:
            rq = dq.re_quantize_matmul(layer.weight, layer.scale, zero_point=layer.zero_point)
            put("requant_weight", rq[0])
            put("requant_scale", rq[1])
            if len(rq) > 2:
                put("requant_zero_point", rq[2])
        xs = make_inputs(case)
        for i, x in enumerate(xs):
            put(f"x_{i}", x)
            put(f"y_{i}", layer(x))
    meta = dict(name=name, kind=case["kind"], dtype=case["dtype"], cfg=case["cfg"], deq=G.deq_fields(dq),
                codebook_steps=dq.codebook_steps, forward_func=layer.forward_func.__name__, n_inputs=len(xs), tensors=tensors,
                geometry={k: case[k] for k in ("K", "N", "cin", "cout", "k", "V", "D") if k in case})
    np.savez_compressed(os.path.join(OUT_DIR, f"cb_{name}.npz"), **arrays)
    with open(os.path.join(OUT_DIR, f"cb_{name}.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", name, {k: v["shape"] for k, v in tensors.items() if k in ("weight", "scale")}, meta["forward_func"])


def verify():
    """Build the reference layer for each stored config, replace its tensors by the stored ones, run the reference forward on the
    stored inputs and require the stored outputs bit for bit."""
    bad = 0
    for case in CASES:
        name = case["name"]
        z = np.load(os.path.join(HERE, f"cb_{name}.npz"))
        with open(os.path.join(HERE, f"cb_{name}.json")) as f:
            meta = json.load(f)
        layer = quantize(case)
        assert G.deq_fields(layer.sdnq_dequantizer) == meta["deq"], name
        for k in ("weight", "scale", "zero_point", "svd_up", "svd_down", "bias"):
            info = meta["tensors"][k]
            if info["shape"] is None:
                assert getattr(layer, k, None) is None, (name, k)
                continue
            t = G.from_np(z[k], info["dtype"])
            if list(t.stride()) != info["stride"]:
                t = torch.empty_strided(tuple(t.shape), tuple(info["stride"]), dtype=t.dtype).copy_(t)
            setattr(layer, k, torch.nn.Parameter(t, requires_grad=False))
        with torch.no_grad():
            for i in range(meta["n_inputs"]):
                x = G.from_np(z[f"x_{i}"], meta["tensors"][f"x_{i}"]["dtype"])
                ya, _ = G.to_np(layer(x))
                ok = np.array_equal(ya, z[f"y_{i}"])
                bad += not ok
                print("verify", name, i, "OK" if ok else f"MISMATCH {(ya != z[f'y_{i}']).sum()} elements")
    print("verify done, mismatching outputs:", bad)
    return bad


def regen_check():
    """Regenerate every fixture into a temp dir and compare array by array with the tracked files."""
    import tempfile
    global OUT_DIR
    OUT_DIR = tempfile.mkdtemp(prefix="sdnq_golden_cb_")
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
