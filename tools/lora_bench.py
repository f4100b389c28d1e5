#!/usr/bin/env python3
"""Trainable low-rank adapters on frozen quantized Linear layers (sdnq_amd.lora) on the problems of tools/train_linear_bench.py: bf16
layers with int8 row-wise weights on the w8a8 forward, ranks 16 and 64.

 (a) "lowrank_add": ops.lowrank_add alone; bytes_per_s is the algorithm's minimum, one read and one write of y = 4 M N bytes, over the
     measured time.
 (b) "lowrank_grad": ops.lowrank_grad(dY, t) (grad_up: reduces over the tokens, P = N) against torch.mm(dY.t(), t).
 (c) "layer": forward + backward of the adapter layer -- gradients for the input and both factors -- against what a user assembles
     without it: the same quantized layer under sdnq_amd.enable_input_grad plus ``scale * (x @ down.t()) @ up.t()`` through torch autograd.

Everything is timed as hipGraph replays (no host launch cost in the numbers): a graph of `--iters` calls, device events around one replay,
`--rounds` rounds alternating the contenders; median and min per call.  "spread" is (max - min) / median over the torch contender's own
windows, the run-to-run spread of this box; the tool fails only where (c) is slower than the composition by more than that.  One JSON
line per measurement, appended to --out.
Usage: python tools/lora_bench.py [--out profiles/lora_bench.jsonl] [--iters 10] [--rounds 7] [--only add|grad|layer]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import ops, training  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.train_linear_bench import DEV, PROBLEMS, emit  # noqa: E402

RANKS = (16, 64)
BF = torch.bfloat16


def med(v):
    return round(statistics.median(v), 2)


def spread_of(v):
    return round((max(v) - min(v)) / statistics.median(v), 4)


def bench_add(out, iters, rounds):
    seen = set()
    for m, _, n in PROBLEMS:
        for rank in RANKS:
            if (m, n, rank) in seen:
                continue
            seen.add((m, n, rank))
            g = torch.Generator(device=DEV).manual_seed(m + n + rank)
            t = torch.randn(m, rank, device=DEV, dtype=BF, generator=g)
            up = torch.randn(n, rank, device=DEV, dtype=BF, generator=g) * 0.05
            y = torch.randn(m, n, device=DEV, dtype=BF, generator=g)
            ref = y.float() + 0.5 * (t.float() @ up.float().t())
            got = ops.lowrank_add(t, up, y.clone(), 0.5).float()
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err <= 2.0 ** -8, ("lowrank_add", m, n, rank, err)            # one bf16 rounding
            v = race({"add": lambda: ops.lowrank_add(t, up, y, 0.0)}, 3 * iters, rounds)["add"]   # scale 0: y keeps its values over the replays
            emit(out, dict(bench="lowrank_add", tokens=m, n=n, rank=rank, dtype="bf16", lowrank_add_us=med(v), lowrank_add_min_us=round(min(v), 2),
                           spread=spread_of(v), min_bytes=4 * m * n, bytes_per_s=round(4 * m * n / (med(v) * 1e-6)),
                           device=torch.cuda.get_device_name(0)))
            del t, up, y, ref, got


def bench_grad(out, iters, rounds):
    seen = set()
    for m, _, n in PROBLEMS:
        for rank in RANKS:
            if (m, n, rank) in seen:
                continue
            seen.add((m, n, rank))
            g = torch.Generator(device=DEV).manual_seed(m + n + rank + 1)
            dy = torch.randn(m, n, device=DEV, dtype=BF, generator=g) * 0.01
            t = torch.randn(m, rank, device=DEV, dtype=BF, generator=g)
            ws = torch.empty(ops.lowrank_grad_workspace_bytes(m, n, rank) + 16, device=DEV, dtype=torch.uint8)
            ref = dy.float().t() @ t.float()
            got = ops.lowrank_grad(dy, t, 1.0, workspace=ws).float()
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err <= 2.0 ** -8, ("lowrank_grad", m, n, rank, err)
            r = race({"hip": lambda: ops.lowrank_grad(dy, t, 1.0, workspace=ws), "torch": lambda: torch.mm(dy.t(), t)}, 3 * iters, rounds)
            emit(out, dict(bench="lowrank_grad", tokens=m, p=n, rank=rank, dtype="bf16", lowrank_grad_us=med(r["hip"]),
                           lowrank_grad_min_us=round(min(r["hip"]), 2), torch_mm_us=med(r["torch"]), torch_mm_min_us=round(min(r["torch"]), 2),
                           spread=spread_of(r["torch"]), ratio=round(med(r["hip"]) / med(r["torch"]), 3), workspace_bytes=ws.numel() - 16,
                           device=torch.cuda.get_device_name(0)))
            del dy, t, ws, ref, got


def quantized(k, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=False, device=DEV, dtype=BF)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, device=DEV, dtype=BF, generator=g) * 0.05)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True))
    return layer


def bench_layer(out, iters, rounds):
    lost = []
    for m, k, n in PROBLEMS:
        for rank in RANKS:
            g = torch.Generator(device=DEV).manual_seed(m + k + n + rank)
            x = torch.randn(m, k, device=DEV, dtype=BF, generator=g).requires_grad_(True)
            dy = torch.randn(m, n, device=DEV, dtype=BF, generator=g) * 0.01
            ours, theirs = torch.nn.Sequential(quantized(k, n, 1)), torch.nn.Sequential(quantized(k, n, 1))
            assert sdnq_amd.add_lora(ours, rank=rank, alpha=2 * rank, seed=3) == 1 and sdnq_amd.enable_input_grad(theirs) == 1
            layer = ours[0]
            with torch.no_grad():
                layer.lora_up.copy_(torch.randn(n, rank, device=DEV, dtype=BF, generator=g) * 0.05)
            down, up = layer.lora_down.detach().clone().requires_grad_(True), layer.lora_up.detach().clone().requires_grad_(True)
            scale = layer.lora_scale

            def lora_step():
                return torch.autograd.grad(ours(x), (x, layer.lora_down, layer.lora_up), dy)

            def composed_step():
                return torch.autograd.grad(theirs(x) + scale * ((x @ down.t()) @ up.t()), (x, down, up), dy)
            for a, b, what in zip(lora_step(), composed_step(), ("grad_input", "grad_down", "grad_up")):
                err = float((a.float() - b.float()).abs().max() / b.float().abs().max())
                assert err <= 2.0 ** -5, (what, m, k, n, rank, err)              # a sanity check: bf16 roundings in two different orders
            r = race({"lora": lora_step, "composed": composed_step}, iters, rounds)
            spread = spread_of(r["composed"])
            line = dict(bench="lora_layer", tokens=m, k=k, n=n, rank=rank, dtype="bf16", weights="int8_rowwise_w8a8",
                        lora_fwd_bwd_us=med(r["lora"]), lora_fwd_bwd_min_us=round(min(r["lora"]), 2), composed_fwd_bwd_us=med(r["composed"]),
                        composed_fwd_bwd_min_us=round(min(r["composed"]), 2), spread=spread,
                        ratio=round(med(r["lora"]) / med(r["composed"]), 3), scratch_bytes=training.scratch_bytes(DEV),
                        device=torch.cuda.get_device_name(0))
            emit(out, line)
            if med(r["lora"]) > med(r["composed"]) * (1 + spread):
                lost.append(line)
            del ours, theirs, layer, x, dy, down, up, r
            training.release_scratch()
            torch.cuda.empty_cache()
    return lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "lora_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("add", "grad", "layer"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    lost = []
    with open(a.out, "a") as f:
        if a.only in (None, "add"):
            bench_add(f, a.iters, a.rounds)
        if a.only in (None, "grad"):
            bench_grad(f, a.iters, a.rounds)
        if a.only in (None, "layer"):
            lost = bench_layer(f, a.iters, a.rounds)
    if lost:
        sys.exit("the adapter layer is slower than the torch composition beyond the run-to-run spread at: "
                 + ", ".join(f"{ln['tokens']}x{ln['k']}x{ln['n']} r{ln['rank']} ({ln['lora_fwd_bwd_us']} vs {ln['composed_fwd_bwd_us']} us)" for ln in lost))


if __name__ == "__main__":
    main()
