#!/usr/bin/env python3
"""The backward of a frozen quantized Conv2d (sdnq_amd.training.QuantizedConvInputGrad) on the convolutions of an SDXL UNet at batch 1,
bf16, int8 row-wise weights with use_quantized_matmul_conv=True and uint4 (group 64) weights without a quantized matmul.  Per problem:

 (a) "backward_us":  this package's backward on the route its static rule picks (training._takes_col2im_route);
     "backward_again_us" is the same graph captured a second time and raced beside it: the run-to-run spread of this box on this shape;
     "gather_route_us" is the backward forced down the gather route -- ops.weight_t into the scratch buffer, ops.im2col_bwd, the float
     GEMM, the permute to NCHW -- whatever the rule says: with (b) it is the measurement the rule rests on;
 (b) "col2im_route_us": the most the kernels from before sdnq_hip_im2col_bwd can do -- dY to NHWC (a torch copy), ops.weight_t, the float32-out
     GEMM over M = B * L_out (ops.linear_float_f32_into) and ops.col2im, the gather half of the transposed convolution;
 (c) "dequant_lib_us": ops.dequant + torch.nn.grad.conv2d_input: what a user could assemble before;
 (d) "lib_resident_us": torch.nn.grad.conv2d_input on a RESIDENT bf16 copy of the weight -- context: it spends the memory (a) saves;
     "im2col_bwd_us": sdnq_hip_im2col_bwd alone; bytes = dY read + U written, and the resulting bytes_per_s.

Everything is timed as hipGraph replays (no host launch cost in the numbers): a graph of `--iters` calls, device events around one replay,
`--rounds` rounds alternating the contenders; medians per call.  "spread" is (max - min) / median over the windows of (a) and its
repeat.  The tool fails where (a) is slower than (b) by more than that shape's spread; against (c) and (d) nothing is asserted -- the
library may win.  One JSON line per problem, written to --out.
Usage: python tools/conv_input_grad_bench.py [--out profiles/conv_input_grad_bench.jsonl] [--iters 10] [--rounds 7]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import linear, ops, training  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.train_linear_bench import DEV, emit  # noqa: E402

FORMATS = {"int8_rowwise_qmm": dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, use_quantized_matmul_conv=True),
           "uint4_g64": dict(weights_dtype="uint4", group_size=64)}
# (name, C_in, C_out, H = W of the input, kernel, stride, padding): the 3x3 ResNet convs of the SDXL UNet, its two down-samplers, a shortcut
SHAPES = [("res_320_320_128", 320, 320, 128, 3, 1, 1), ("res_640_640_64", 640, 640, 64, 3, 1, 1), ("res_1280_1280_32", 1280, 1280, 32, 3, 1, 1),
          ("res_320_640_64", 320, 640, 64, 3, 1, 1), ("res_640_1280_32", 640, 1280, 32, 3, 1, 1), ("res_2560_1280_32", 2560, 1280, 32, 3, 1, 1),
          ("res_1920_640_64", 1920, 640, 64, 3, 1, 1), ("res_960_320_128", 960, 320, 128, 3, 1, 1),
          ("down_320_128", 320, 320, 128, 3, 2, 1), ("down_640_64", 640, 640, 64, 3, 2, 1), ("shortcut_320_640_64", 320, 640, 64, 1, 1, 0)]


def col2im_route(qw, dy, cin, hw, k, s, p, scratch):
    """grad_x [B][C_in][H][W] by the kernels of the transposed convolution: cols[(b, oh, ow)][(ci, kpos)] = dY . W in float32, then every
    input pixel gathers the taps that reach it (ops.col2im), one rounding."""
    b, cout, ho, wo = dy.shape
    wt = ops.weight_t(qw, dy.dtype, 0, scratch)                                  # [C_in * kprod][C_out]: the GEMM's [N][K] operand
    dy2d = dy.permute(0, 2, 3, 1).contiguous().view(b * ho * wo, cout)
    cols = torch.empty((b * ho * wo, wt.shape[0]), device=dy.device, dtype=torch.float32)
    ops.linear_float_f32_into(dy2d, wt, cols, 0)
    return ops.col2im(cols, None, dy.dtype, b, cin, (ho, wo), (hw, hw), (k, k), (s, s), (p, p), (1, 1))


def bench(out, iters, rounds):
    lost = []
    for fmt, cfg in FORMATS.items():
        for name, cin, cout, hw, k, s, p in SHAPES:
            g = torch.Generator(device=DEV).manual_seed(cin + cout + hw)
            conv = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=False, device=DEV, dtype=torch.bfloat16)
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, device=DEV, dtype=torch.bfloat16, generator=g) * 0.05)
            layer, _ = sdnq_amd.sdnq_quantize_layer(conv, sdnq_amd.SDNQConfig(quant_conv=True, **cfg))
            assert training.input_grad_unsupported_reason(layer, convs=True) is None, (fmt, name)
            qw = linear._state(layer).qw
            ho = (hw + 2 * p - k) // s + 1
            dy = torch.randn(1, cout, ho, ho, device=DEV, dtype=torch.bfloat16, generator=g) * 0.01
            shape = (1, cin, hw, hw)
            w_float = ops.dequant(qw, torch.bfloat16, 0).view(cout, cin, k, k)                 # resident for (d)
            ctx = type("Ctx", (), {"layer": layer, "input_shape": shape, "needs_input_grad": (False, True, False), "bias_dtype": None})()

            def backward():
                return training.QuantizedConvInputGrad.backward(ctx, dy)[1]
            backward()                                                                         # sizes the scratch buffers
            route_scratch = training.scratch_bytes(DEV)

            def gather():
                training.CONV_GRAD_ROUTE = "gather"
                try:
                    return backward()
                finally:
                    training.CONV_GRAD_ROUTE = None
            gather()
            scratch = (sdnq_amd.scratch.take(DEV, "input-gradient scratch", 2 * qw.n * qw.k, "operand")[0].view(torch.bfloat16), None)
            ubuf = sdnq_amd.scratch.take(DEV, "input-gradient scratch", 2 * hw * hw * k * k * cout, "unfolded")[0].view(torch.bfloat16)

            def route_b():
                return col2im_route(qw, dy, cin, hw, k, s, p, scratch)

            def dequant_lib():
                return torch.nn.grad.conv2d_input(shape, ops.dequant(qw, torch.bfloat16, 0).view(cout, cin, k, k), dy, stride=s, padding=p)

            def lib_resident():
                return torch.nn.grad.conv2d_input(shape, w_float, dy, stride=s, padding=p)
            ref = lib_resident().float()
            for what, got in (("backward", backward()), ("gather_route", gather()), ("col2im_route", route_b())):
                err = float((got.float() - ref).abs().max() / ref.abs().max())
                assert got.shape == ref.shape and err <= 2 * 2.0 ** -7, (what, fmt, name, err)   # two bf16 roundings of two summation orders
            t = race({"backward": backward, "col2im_route": route_b, "dequant_lib": dequant_lib, "backward_again": backward,
                      "lib_resident": lib_resident, "gather_route": gather,
                      "im2col_bwd": lambda: ops.im2col_bwd(dy, (hw, hw), (k, k), (s, s), (p, p), (1, 1), out=ubuf)}, iters, rounds)
            med = {key: round(statistics.median(v), 2) for key, v in t.items()}
            both = t["backward"] + t["backward_again"]
            spread = round((max(both) - min(both)) / statistics.median(both), 4)
            nbytes = dy.numel() * 2 + hw * hw * k * k * cout * 2
            line = dict(bench="conv_input_grad", format=fmt, name=name, c_in=cin, c_out=cout, input=hw, kernel=k, stride=s, padding=p, dtype="bf16",
                        backward_us=med["backward"], backward_min_us=round(min(t["backward"]), 2), backward_again_us=med["backward_again"],
                        route="col2im" if training._takes_col2im_route(1, k * k, (s, s), hw * hw) else "gather", gather_route_us=med["gather_route"],
                        col2im_route_us=med["col2im_route"], col2im_route_min_us=round(min(t["col2im_route"]), 2),
                        dequant_lib_us=med["dequant_lib"], lib_resident_us=med["lib_resident"], im2col_bwd_us=med["im2col_bwd"],
                        im2col_bwd_bytes=nbytes, im2col_bwd_bytes_per_s=round(nbytes / (med["im2col_bwd"] * 1e-6)), spread=spread,
                        backward_vs_col2im_route=round(med["backward"] / med["col2im_route"], 3),
                        backward_vs_dequant_lib=round(med["backward"] / med["dequant_lib"], 3),
                        backward_vs_lib_resident=round(med["backward"] / med["lib_resident"], 3),
                        scratch_bytes=route_scratch, resident_float_bytes=2 * qw.n * qw.k, device=torch.cuda.get_device_name(0))
            emit(out, line)
            if med["backward"] > med["col2im_route"] * (1 + spread):
                lost.append(line)
            del conv, layer, qw, dy, w_float, scratch, ubuf, ref, ctx
            training.release_scratch()
            torch.cuda.empty_cache()
    return lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "conv_input_grad_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_input_grad_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        lost = bench(f, a.iters, a.rounds)
    if lost:
        sys.exit("the backward is slower than weight_t + float32 GEMM + col2im beyond the run-to-run spread at: "
                 + ", ".join(f"{ln['format']} {ln['name']}" for ln in lost))


if __name__ == "__main__":
    main()
