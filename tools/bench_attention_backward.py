#!/usr/bin/env python3
"""Quantized attention forward + backward (sdnq_hip_atten_with_backward) against torch's bf16 SDPA forward + backward, per attention call
of one SDXL UNet step (shapes.sdxl_unet_attentions) and one FLUX.1-dev step (shapes.flux_dev_attentions), plus the 10 x 4096^2 x 64 goal
shape.  Device events around `reps` eager iterations after `warmup` ones (steady state), the median of `rounds`; one JSON line per call.
Usage: python tools/bench_attention_backward.py [--out profiles/attention_backward_bench.jsonl] [--reps 10] [--rounds 5]
Per-kernel times: rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/bench_attention_backward.py --reps 3 --rounds 1"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import shapes  # noqa: E402
from sdnq_amd.attention import sdnq_hip_atten_with_backward  # noqa: E402


def timed(fn, warmup, reps, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(res)  # us per forward + backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "attention_backward_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    calls = [("goal", 10, 4096, 4096, 64, 1)] + [("sdxl." + c[0],) + c[1:] for c in shapes.sdxl_unet_attentions()] + \
            [("flux." + c[0],) + c[1:] for c in shapes.flux_dev_attentions()]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        for name, h, qn, kn, d, rep in calls:
            g = torch.Generator(device=dev).manual_seed(0)
            q = torch.randn(1, h, qn, d, device=dev, dtype=torch.bfloat16, generator=g).requires_grad_(True)
            k = torch.randn(1, h, kn, d, device=dev, dtype=torch.bfloat16, generator=g).requires_grad_(True)
            v = torch.randn(1, h, kn, d, device=dev, dtype=torch.bfloat16, generator=g).requires_grad_(True)
            do = torch.randn(1, h, qn, d, device=dev, dtype=torch.bfloat16, generator=g)

            def run(attn):
                def step():
                    out = attn(q, k, v)
                    torch.autograd.backward(out, do, inputs=[q, k, v])
                return step
            ours = timed(run(sdnq_hip_atten_with_backward), a.warmup, a.reps, a.rounds)
            sdpa = timed(run(torch.nn.functional.scaled_dot_product_attention), a.warmup, a.reps, a.rounds)
            line = dict(call=name, heads=h, q_len=qn, kv_len=kn, head_dim=d, repeat=rep, sdnq_fwd_bwd_us=round(ours, 1),
                        torch_sdpa_bf16_fwd_bwd_us=round(sdpa, 1), ratio=round(ours / sdpa, 3), device=torch.cuda.get_device_name(0))
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
