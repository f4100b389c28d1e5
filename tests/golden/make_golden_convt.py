#!/usr/bin/env python3
"""Golden vectors for the transposed-convolution forwards (sdnq_amd.conv_transpose, csrc/convt.hip), made by RUNNING the reference's
quantizer (`sdnq_quantize_layer` under `quant_conv=True`) and its `quantized_conv_transpose_{1,2,3}d_forward` on the CPU, with the
environment switches and the fake `diffusers` of make_golden.py.  Files are ``convt_<name>.npz`` / ``.json`` and hold DATA only:

  w_float                         the float weight [C_in, C_out / groups, *kernel] in the case's dtype
  weight, scale, zero_point       the stored tensors of the quantized layer (packed formats: the flat packed words)
  w_deq                           SDNQDequantizer.__call__ of the reference on them, [C_in, C_out / groups, *kernel] in the result dtype
  bias, x, y                      bias (or absent), the input and the reference forward's output
  the json: the layer's constructor arguments, the quantization config, the dequantizer's fields (`deq`), the forward's
  `output_size` argument (or null) and every tensor's dtype tag / shape.
``convt_checkpoint_tiny/`` is a two-layer model (Linear + ConvTranspose2d) quantized, saved and re-loaded by the reference
(`save_sdnq_model` / `load_sdnq_model`), with the re-loaded model's input / output on one batch (`io.npz`).

The cases are the smallest at which each piece can go wrong: the column scale layout and the square grouped one (zero point), one tap
per output (k = stride), conv groups, dilation with `output_size=`, 1-D with a long kernel, 3-D with per-axis strides and no bias, a
packed format, 16-bit scales (`apply_sdnq_options_to_model(dequantize_fp32=False)`).

Usage:  python tests/golden/make_golden_convt.py [case ...]
        python tests/golden/make_golden_convt.py --verify     # stored tensors -> the reference's quantizer, dequantizer and forward, bit for bit
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets the environment switches, installs the fake diffusers, imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdnq import SDNQConfig, sdnq_quantize_layer  # noqa: E402  (the reference)

CKPT = os.path.join(HERE, "convt_checkpoint_tiny")
BASE = dict(quant_conv=True, minimum_allowed_numel=1024)
CASES = [
    dict(name="2d_int8_bf16", nd=2, dtype="bf16", cin=64, cout=32, k=4, layer=dict(stride=2, padding=1), batch=2, size=(9, 7),
         cfg=dict(weights_dtype="int8")),
    dict(name="2d_sq_uint4_grouped_f16", nd=2, dtype="f16", cin=64, cout=64, k=3, layer=dict(stride=2, padding=1, output_padding=1), batch=2,
         size=(9, 7), cfg=dict(weights_dtype="uint4")),
    dict(name="2d_k2s2_uint8_f32", nd=2, dtype="f32", cin=64, cout=64, k=2, layer=dict(stride=2), batch=2, size=(8, 8),
         cfg=dict(weights_dtype="uint8", group_size=-1)),
    dict(name="2d_groups2_int8_bf16", nd=2, dtype="bf16", cin=64, cout=32, k=4, layer=dict(stride=2, padding=1, groups=2), batch=2,
         size=(9, 7), cfg=dict(weights_dtype="int8")),
    dict(name="2d_dil_outsize_f16", nd=2, dtype="f16", cin=32, cout=32, k=3, layer=dict(stride=3, padding=2, dilation=2), batch=2,
         size=(5, 6), cfg=dict(weights_dtype="int8"), output_size=(13, 17)),
    dict(name="1d_fp8_bf16", nd=1, dtype="bf16", cin=64, cout=48, k=16, layer=dict(stride=8, padding=4), batch=2, size=(11,),
         cfg=dict(weights_dtype="float8_e4m3fn")),
    dict(name="3d_int8_nobias_bf16", nd=3, dtype="bf16", cin=32, cout=16, k=3, layer=dict(stride=(1, 2, 2), padding=1, bias=False), batch=1,
         size=(3, 5, 6), cfg=dict(weights_dtype="int8")),
    dict(name="2d_int5_bf16", nd=2, dtype="bf16", cin=64, cout=32, k=4, layer=dict(stride=2, padding=1), batch=2, size=(9, 7),
         cfg=dict(weights_dtype="int5")),
    dict(name="2d_int8_lpscale_bf16", nd=2, dtype="bf16", cin=64, cout=32, k=4, layer=dict(stride=2, padding=1), batch=2, size=(9, 7),
         cfg=dict(weights_dtype="int8"), lpscale=True),
]
CTOR = {1: torch.nn.ConvTranspose1d, 2: torch.nn.ConvTranspose2d, 3: torch.nn.ConvTranspose3d}


def make_layer(case):
    g = torch.Generator().manual_seed(zlib.crc32(("convt_" + case["name"]).encode()))
    layer = CTOR[case["nd"]](case["cin"], case["cout"], case["k"], **case["layer"])
    with torch.no_grad():
        w = torch.randn(layer.weight.shape, generator=g) * 0.05
        w[3] *= 6.0  # an outlier input channel
        layer.weight.copy_(w)
        if layer.bias is not None:
            layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.1)
    x = torch.randn(case["batch"], case["cin"], *case["size"], generator=g)
    dt = G.TORCH_DT[case["dtype"]]
    return layer.to(dt), x.to(dt)


def quantize(case, layer):
    """The reference's quantized layer of `layer` (modified in place, as the reference does)."""
    q = sdnq_quantize_layer(layer, SDNQConfig(**BASE, **case["cfg"]))[0]
    assert hasattr(q, "sdnq_dequantizer"), case["name"]
    if case.get("lpscale"):
        from sdnq.loader import apply_sdnq_options_to_model
        holder = torch.nn.Sequential(q)
        holder.quantization_config = SDNQConfig(**BASE, **case["cfg"])
        apply_sdnq_options_to_model(holder, dequantize_fp32=False)
        assert q.scale.dtype == G.TORCH_DT[case["dtype"]]
    return q


def run_reference(case, w_float, bias, x):
    layer = CTOR[case["nd"]](case["cin"], case["cout"], case["k"], **case["layer"]).to(w_float.dtype)
    with torch.no_grad():
        layer.weight.copy_(w_float)
        if bias is not None:
            layer.bias.copy_(bias)
    q = quantize(case, layer)
    with torch.no_grad():
        w_deq = q.sdnq_dequantizer(q.weight, q.scale, q.zero_point, q.svd_up, q.svd_down)
        y = q(x, output_size=list(case["output_size"])) if case.get("output_size") else q(x)
    res = dict(weight=q.weight.detach(), scale=q.scale.detach(), w_deq=w_deq, y=y)
    if q.zero_point is not None:
        res["zero_point"] = q.zero_point.detach()
    return res, q


def run_case(case):
    layer, x = make_layer(case)
    w_float = layer.weight.detach().clone()
    bias = None if layer.bias is None else layer.bias.detach().clone()
    res, q = run_reference(case, w_float, bias, x)
    tensors = dict(w_float=w_float, x=x, **res)
    if bias is not None:
        tensors["bias"] = bias
    out, info = {}, {}
    for key, t in tensors.items():
        arr, tag = G.to_np(t)
        out[key] = arr
        info[key] = dict(dtype=tag, shape=list(t.shape))
    jl = {k: (list(v) if isinstance(v, tuple) else v) for k, v in case["layer"].items()}
    meta = dict(name=case["name"], nd=case["nd"], dtype=case["dtype"], cin=case["cin"], cout=case["cout"], k=case["k"], layer=jl,
                cfg=dict(BASE, **case["cfg"]), lpscale=bool(case.get("lpscale")), output_size=list(case["output_size"]) if case.get("output_size") else None,
                deq=G.deq_fields(q.sdnq_dequantizer), forward_func=q.forward_func.__name__, tensors=info)
    np.savez_compressed(os.path.join(HERE, f"convt_{case['name']}.npz"), **out)
    with open(os.path.join(HERE, f"convt_{case['name']}.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", case["name"], {k: v["shape"] for k, v in info.items() if k in ("weight", "scale", "y")})


class TinyUp(torch.nn.Module):
    """proj 64 -> 64 on the channel axis, then up: ConvTranspose2d(64, 32, 4, stride 2, padding 1)."""

    def __init__(self, c_in=64, c_out=32):
        super().__init__()
        self.cfg = dict(c_in=c_in, c_out=c_out)
        self.proj = torch.nn.Linear(c_in, c_in)
        self.up = torch.nn.ConvTranspose2d(c_in, c_out, 4, stride=2, padding=1)

    def forward(self, x):
        return self.up(self.proj(x.movedim(1, -1)).movedim(-1, 1))

    def save_pretrained(self, path, max_shard_size=None):  # what ModelMixin.save_pretrained leaves on disk
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(path, "model.safetensors"))
        json.dump(dict(self.cfg), open(os.path.join(path, "config.json"), "w"), indent=1)


def checkpoint_config():
    return SDNQConfig(weights_dtype="int8", quant_conv=True, minimum_allowed_numel=1024, add_skip_keys=False)


def run_checkpoint(out=CKPT):
    import sdnq
    mixin = sdnq.SDNQConfig.__mro__[1]
    mixin.to_json_string = lambda self: json.dumps(self.to_dict(), indent=2, sort_keys=True) + "\n"
    mixin.to_json_file = lambda self, path: open(path, "w", encoding="utf-8").write(self.to_json_string())
    from sdnq import sdnq_post_load_quant
    from sdnq.loader import load_sdnq_model, save_sdnq_model
    torch.manual_seed(20261018)
    model = TinyUp().to(torch.bfloat16)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn_like(p, dtype=torch.float32) * 0.08)
    model = sdnq_post_load_quant(model, torch_dtype=torch.bfloat16, quantization_config=checkpoint_config())
    assert type(model.up).__name__ == "SDNQConvTranspose2d", type(model.up)
    for f in os.listdir(out) if os.path.isdir(out) else []:
        os.remove(os.path.join(out, f))
    save_sdnq_model(model, out)
    loaded = load_sdnq_model(out, model_cls=TinyUp, dtype=torch.bfloat16, device="cpu")
    x = (torch.randn(2, 64, 5, 6) * 1.5).to(torch.bfloat16)
    bits = lambda t: t.detach().contiguous().view(torch.uint16).numpy().copy()  # noqa: E731  (bf16 bit patterns)
    with torch.no_grad():
        y = loaded(x)
    np.savez_compressed(os.path.join(out, "io.npz"), x=bits(x), y=bits(y))
    print("wrote", out, sorted(os.listdir(out)))


def load_case(name):
    with open(os.path.join(HERE, f"convt_{name}.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(HERE, f"convt_{name}.npz"))
    return meta, {k: G.from_np(z[k], i["dtype"]).reshape(i["shape"]) for k, i in meta["tensors"].items()}


def verify():
    bad = 0
    for case in CASES:
        meta, t = load_case(case["name"])
        res, q = run_reference(case, t["w_float"], t.get("bias"), t["x"])
        ok = G.deq_fields(q.sdnq_dequantizer) == meta["deq"]
        bad += not ok
        if not ok:
            print("verify", case["name"], "dequantizer fields MISMATCH")
        for key, r in res.items():
            ok = key in t and r.dtype == t[key].dtype and np.array_equal(G.to_np(r)[0], G.to_np(t[key])[0])
            bad += not ok
            if not ok:
                print("verify", case["name"], key, "MISMATCH")
        print("verify", case["name"], len(res), "tensors")
    from sdnq.loader import load_sdnq_model
    loaded = load_sdnq_model(CKPT, model_cls=TinyUp, dtype=torch.bfloat16, device="cpu")
    io = np.load(os.path.join(CKPT, "io.npz"))
    with torch.no_grad():
        y = loaded(torch.from_numpy(io["x"].copy()).view(torch.bfloat16))
    ok = np.array_equal(y.contiguous().view(torch.uint16).numpy(), io["y"])
    bad += not ok
    print("verify checkpoint", "OK" if ok else "MISMATCH")
    print("verify done, mismatches:", bad)
    return bad


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--verify" in sys.argv[1:]:
        sys.exit(1 if verify() else 0)
    only = sys.argv[1:]
    for c in CASES:
        if not only or c["name"] in only:
            run_case(c)
    if not only or "checkpoint" in only:
        run_checkpoint()
