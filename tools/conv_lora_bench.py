#!/usr/bin/env python3
"""Low-rank adapters on frozen quantized Conv2d layers (sdnq_amd.lora, add_lora(..., convs=True)) on the eleven conv problems of
tools/conv_input_grad_bench.py: bf16, batch 1, int8 row-wise weights with use_quantized_matmul_conv=True, ranks 16 and 64.

 (a) "kernels": ops.conv_lowrank_down against ops.im2col + ops.lowrank_down, and ops.conv_lowrank_grad against ops.im2col +
     ops.lowrank_grad -- what the library could do before the implicit kernels, and the reason they exist.  Each implicit kernel is
     captured twice ("..._again_us") and raced beside itself: "spread" is (max - min) / median over those windows, the run-to-run spread of
     this box on this problem.  CONDITION: neither kernel is slower than its composition by more than that spread; the tool fails where
     one is (sdnq_amd.lora takes the implicit kernels on every layer).
 (b) "layer": forward + backward of the adapter layer -- gradients for the input and both factors -- against the same layer under
     sdnq_amd.enable_input_grad(convs=True) plus ``scale * F.conv2d(F.conv2d(x, A, stride, padding), B)`` through torch autograd.  Reported
     whichever way it falls; nothing is asserted on it.

Everything is timed as hipGraph replays (no host launch cost in the numbers): a graph of `--iters` calls, device events around one replay,
`--rounds` rounds alternating the contenders; medians per call.  One JSON line per measurement, written to --out.
Usage: python tools/conv_lora_bench.py [--out profiles/conv_lora_bench.jsonl] [--iters 10] [--rounds 7] [--only kernels|layer]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import ops, training  # noqa: E402
from tools.conv_input_grad_bench import SHAPES  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.train_linear_bench import DEV, emit  # noqa: E402

RANKS = (16, 64)
BF = torch.bfloat16
INT8 = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, use_quantized_matmul_conv=True, quant_conv=True)


def med(v):
    return round(statistics.median(v), 2)


def spread_of(*vs):
    both = [t for v in vs for t in v]
    return round((max(both) - min(both)) / statistics.median(both), 4)


def bench_kernels(out, iters, rounds):
    lost = []
    for name, cin, _, hw, k, s, p in SHAPES:
        geo = ((k, k), (s, s), (p, p), (1, 1))
        ho = (hw + 2 * p - k) // s + 1
        m, kk = ho * ho, cin * k * k
        for rank in RANKS:
            g = torch.Generator(device=DEV).manual_seed(cin + hw + rank)
            x = torch.randn(1, cin, hw, hw, device=DEV, dtype=BF, generator=g)
            down = torch.randn(rank, kk, device=DEV, dtype=BF, generator=g) * 0.02
            gt = torch.randn(m, rank, device=DEV, dtype=BF, generator=g) * 0.01
            ws = torch.empty(ops.conv_lowrank_grad_workspace_bytes(x.shape, *geo, rank) + 16, device=DEV, dtype=torch.uint8)
            ws2 = torch.empty(ops.lowrank_grad_workspace_bytes(m, kk, rank) + 16, device=DEV, dtype=torch.uint8)

            def implicit_down():
                return ops.conv_lowrank_down(x, down, *geo)[0]

            def unfold_down():
                return ops.lowrank_down(ops.im2col(x, *geo)[0], down)

            def implicit_grad():
                return ops.conv_lowrank_grad(x, gt, *geo, 1.0, workspace=ws)

            def unfold_grad():
                return ops.lowrank_grad(ops.im2col(x, *geo)[0], gt, 1.0, out_t=True, workspace=ws2)
            for what, a, b in (("down", implicit_down(), unfold_down()), ("grad", implicit_grad(), unfold_grad())):
                err = float((a.float() - b.float()).abs().max() / b.float().abs().max())
                assert a.shape == b.shape and err <= 2.0 ** -7, (what, name, rank, err)    # one bf16 rounding of two summation orders
            t = race({"down": implicit_down, "unfold_down": unfold_down, "grad": implicit_grad, "unfold_grad": unfold_grad,
                      "down_again": implicit_down, "grad_again": implicit_grad}, iters, rounds)
            line = dict(bench="conv_lora_kernels", name=name, c_in=cin, input=hw, kernel=k, stride=s, padding=p, rank=rank, dtype="bf16",
                        positions=m, k=kk,
                        conv_lowrank_down_us=med(t["down"]), conv_lowrank_down_again_us=med(t["down_again"]),
                        im2col_lowrank_down_us=med(t["unfold_down"]), down_spread=spread_of(t["down"], t["down_again"]),
                        down_ratio=round(med(t["down"]) / med(t["unfold_down"]), 3),
                        conv_lowrank_grad_us=med(t["grad"]), conv_lowrank_grad_again_us=med(t["grad_again"]),
                        im2col_lowrank_grad_us=med(t["unfold_grad"]), grad_spread=spread_of(t["grad"], t["grad_again"]),
                        grad_ratio=round(med(t["grad"]) / med(t["unfold_grad"]), 3),
                        unfolded_bytes=2 * m * kk, x_bytes=2 * x.numel(), workspace_bytes=ws.numel() - 16,
                        device=torch.cuda.get_device_name(0))
            emit(out, line)
            if (med(t["down"]) > med(t["unfold_down"]) * (1 + line["down_spread"])
                    or med(t["grad"]) > med(t["unfold_grad"]) * (1 + line["grad_spread"])):
                lost.append(line)
            del x, down, gt, ws, ws2, t
            torch.cuda.empty_cache()
    return lost


def quantized(cin, cout, k, s, p, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=False, device=DEV, dtype=BF)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device=DEV, dtype=BF, generator=g) * 0.05)
    layer, _ = sdnq_amd.sdnq_quantize_layer(conv, sdnq_amd.SDNQConfig(**INT8))
    return layer


def bench_layer(out, iters, rounds):
    conv2d = torch.nn.functional.conv2d
    for name, cin, cout, hw, k, s, p in SHAPES:
        for rank in RANKS:
            g = torch.Generator(device=DEV).manual_seed(cin + cout + hw + rank)
            x = torch.randn(1, cin, hw, hw, device=DEV, dtype=BF, generator=g).requires_grad_(True)
            ours, theirs = torch.nn.Sequential(quantized(cin, cout, k, s, p, 1)), torch.nn.Sequential(quantized(cin, cout, k, s, p, 1))
            assert sdnq_amd.add_lora(ours, rank=rank, alpha=2 * rank, seed=3, convs=True) == 1
            assert sdnq_amd.enable_input_grad(theirs, convs=True) == 1
            layer = ours[0]
            with torch.no_grad():
                layer.lora_up.copy_(torch.randn(layer.lora_up.shape, device=DEV, dtype=BF, generator=g) * 0.05)
                dy = torch.randn_like(ours(x)) * 0.01
            down, up = layer.lora_down.detach().clone().requires_grad_(True), layer.lora_up.detach().clone().requires_grad_(True)
            scale = layer.lora_scale

            def lora_step():
                return torch.autograd.grad(ours(x), (x, layer.lora_down, layer.lora_up), dy)

            def composed_step():
                return torch.autograd.grad(theirs(x) + scale * conv2d(conv2d(x, down, stride=s, padding=p), up), (x, down, up), dy)
            for a, b, what in zip(lora_step(), composed_step(), ("grad_input", "grad_down", "grad_up")):
                err = float((a.float() - b.float()).abs().max() / b.float().abs().max())
                assert err <= 2.0 ** -5, (what, name, rank, err)                  # a sanity check: bf16 roundings in two different orders
            r = race({"lora": lora_step, "composed": composed_step}, iters, rounds)
            emit(out, dict(bench="conv_lora_layer", name=name, c_in=cin, c_out=cout, input=hw, kernel=k, stride=s, padding=p, rank=rank,
                           dtype="bf16", weights="int8_rowwise_qmm", lora_fwd_bwd_us=med(r["lora"]), lora_fwd_bwd_min_us=round(min(r["lora"]), 2),
                           composed_fwd_bwd_us=med(r["composed"]), composed_fwd_bwd_min_us=round(min(r["composed"]), 2),
                           spread=spread_of(r["composed"]), ratio=round(med(r["lora"]) / med(r["composed"]), 3),
                           scratch_bytes=training.scratch_bytes(DEV), device=torch.cuda.get_device_name(0)))
            del ours, theirs, layer, x, dy, down, up, r
            training.release_scratch()
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "conv_lora_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("kernels", "layer"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_lora_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    lost = []
    with open(a.out, "w") as f:
        if a.only in (None, "kernels"):
            lost = bench_kernels(f, a.iters, a.rounds)
        if a.only in (None, "layer"):
            bench_layer(f, a.iters, a.rounds)
    if lost:
        sys.exit("an implicit kernel is slower than ops.im2col + its Linear kernel beyond the run-to-run spread at: "
                 + ", ".join(f"{ln['name']} r{ln['rank']} (down {ln['down_ratio']}, grad {ln['grad_ratio']})" for ln in lost))


if __name__ == "__main__":
    main()
