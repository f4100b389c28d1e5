#!/usr/bin/env python3
"""The transposed-conv forward (sdnq_amd.conv_transpose: dequantize into the GEMM operand, float GEMM with a float32 store, col2im) against
the library convolution on the same layer, bfloat16, int8 weights with one scale per column, batch 1:

  hip        the module's forward: im2col (1 x 1), sdnq_hip_dequant_convt, sdnq_hip_linear_float_f32out per conv group, sdnq_hip_col2im
  lib        this build's dequantizer (SDNQDequantizer.__call__) followed by torch.nn.functional.conv_transposeNd -- what a model computes per
             call when it keeps the reference's forward.  NOTE the handicap: that dequantizer is sdnq_hip_dequant_convt into [P][C_in] plus a
             transpose copy back to the module layout, two passes over the weight where an elementwise dequantize needs one
             (`lib_deq_us` is its share); `lib_conv` is the side without it
  lib_conv   torch.nn.functional.conv_transposeNd alone on an already dequantized weight (the convolution's share of `lib`)

Shapes (stated here, not measured from a model run):
  cascade_1280 / cascade_640   ConvTranspose2d(c, c, 2, stride 2), the square k 2 / s 2 up-sampler form of Stable Cascade / Wuerstchen
                               up-blocks, at the two wide block widths of Stable Cascade's Stage B (block_out_channels 320, 640, 1280,
                               1280) and the latent sizes those levels have for a 1024 x 1024 image (256 / 8 = 32 and 256 / 4 = 64)
  unet_up_k4s2                 diffusers Upsample2D(use_conv_transpose=True): ConvTranspose2d(c, c, 4, stride 2, padding 1), c = 320 (the
                               first block width of the SD UNets) at 64 x 64
  vocoder_k16s8                HiFi-GAN V1's first up-sampler: ConvTranspose1d(512, 256, 16, stride 8, padding 4) on 256 mel frames

Timing: EAGER calls on the default stream (Python and ctypes launch overhead included on every side), `--iters` calls between two device events, `--rounds` rounds with the contenders in alternation
after a warm-up round; median and min per call.  flop = 2 * M * C_in * P (the GEMM's; the library convolution needs the same products),
one JSON line per shape, written to --out.  No ratio is asserted.
Usage: python tools/convt_bench.py [--out profiles/convt_bench.jsonl] [--iters 200] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [
    dict(name="cascade_1280", nd=2, cin=1280, cout=1280, k=2, layer=dict(stride=2), size=(32, 32)),
    dict(name="cascade_640", nd=2, cin=640, cout=640, k=2, layer=dict(stride=2), size=(64, 64)),
    dict(name="unet_up_k4s2", nd=2, cin=320, cout=320, k=4, layer=dict(stride=2, padding=1), size=(64, 64)),
    dict(name="vocoder_k16s8", nd=1, cin=512, cout=256, k=16, layer=dict(stride=8, padding=4), size=(256,)),
]
CTOR = {1: torch.nn.ConvTranspose1d, 2: torch.nn.ConvTranspose2d}
FUNC = {1: torch.nn.functional.conv_transpose1d, 2: torch.nn.functional.conv_transpose2d}


def race(fns: dict, iters, rounds):
    """{name: (median us, min us)} per call; the contenders alternate, the first round is a warm-up."""
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) * 1000.0 / iters)
    return {k: (statistics.median(t), min(t)) for k, t in times.items()}


@torch.no_grad()
def bench(shape, iters, rounds):
    torch.manual_seed(1)
    layer = CTOR[shape["nd"]](shape["cin"], shape["cout"], shape["k"], **shape["layer"]).to(torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, quant_conv=True)
    mod = sdnq_amd.sdnq_quantize_layer(layer, cfg)[0].to(DEV)
    x = torch.randn(1, shape["cin"], *shape["size"], device=DEV).to(torch.bfloat16)
    dq = mod.sdnq_dequantizer
    kw = shape["layer"]

    def lib_conv(w):
        return FUNC[shape["nd"]](x, w, mod.bias, kw.get("stride", 1), kw.get("padding", 0), 0, 1, 1)

    def lib():
        return lib_conv(dq(mod.weight, mod.scale, mod.zero_point, None, None))
    wd = dq(mod.weight, mod.scale, mod.zero_point, None, None)
    y, y_lib = mod(x), lib()
    err = (y.float() - y_lib.float()).abs().max().item() / y_lib.float().abs().max().item()
    assert y.shape == y_lib.shape and err <= 2 * 2.0 ** -7, f"{shape['name']}: the two sides differ by {err} of the output's magnitude"
    res = race({"hip": lambda: mod(x), "lib": lib, "lib_conv": lambda: lib_conv(wd),
                "lib_deq": lambda: dq(mod.weight, mod.scale, mod.zero_point, None, None)}, iters, rounds)
    m = 1
    for s in shape["size"]:
        m *= s
    p_cols = shape["cout"] * shape["k"] ** shape["nd"]
    line = dict(bench="conv_transpose_forward", name=shape["name"], dtype="bfloat16", weights_dtype="int8", c_in=shape["cin"], c_out=shape["cout"],
                kernel=shape["k"], input=list(shape["size"]), output=list(y.shape[2:]), **{k: v for k, v in kw.items()},
                gemm_m=m, gemm_n=p_cols, gemm_k=shape["cin"], flop=2 * m * p_cols * shape["cin"], max_diff_over_max=round(err, 6),
                iters=iters, rounds=rounds)
    for k, (med, lo) in res.items():
        line[k + "_us"], line[k + "_min_us"] = round(med, 2), round(lo, 2)
    line["lib_over_hip"] = round(res["lib"][0] / res["hip"][0], 3)
    line["lib_conv_over_hip"] = round(res["lib_conv"][0] / res["hip"][0], 3)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "convt_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for shape in SHAPES:
            line = bench(shape, a.iters, a.rounds)
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
