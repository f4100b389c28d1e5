#!/usr/bin/env python3
"""LoRA dropout fused into the adapter kernels (sdnq_amd.lora, add_lora(dropout=p)) on the eight problems of tools/train_linear_bench.py:
bf16 layers with int8 row-wise weights on the w8a8 forward, ranks 16 and 64, p = 0.1.

 (a) "kernel": each of the three dropout kernels against its plain sibling on the same operands -- ops.lowrank_down_dropout(x, down) /
     ops.lowrank_down, ops.lowrank_grad_dropout(x, g_t) / ops.lowrank_grad (grad_down: P = K), ops.lowrank_add_dropout(g_t, down^T, gi) /
     ops.lowrank_add (grad_input's term: N = K).  A fixed (seed, offset) needs no host draw, so these are timed as hipGraph replays like
     tools/lora_bench.py: a graph of 3 x `--iters` calls, `--rounds` rounds alternating the two.  ratio = dropout / plain: what the
     Philox arithmetic costs on a kernel that is otherwise bound by its memory traffic.
 (b) "layer": forward + backward of the adapter layer in train() -- gradients for the input and both factors -- at dropout = 0.1 against
       plain     the same layer at dropout = 0: ratio_to_plain is the price of the feature;
       composed  what a user can assemble without it: the quantized layer under sdnq_amd.enable_input_grad plus
                 ``scale * (F.dropout(x, p) @ down.t()) @ up.t()`` through torch autograd.
     A stochastic step does not capture (the offset is drawn on the host), so all three are timed EAGER: device events around `--iters`
     calls, `--rounds` rounds alternating the contenders; host launch cost is in all three numbers.

Medians per call; "spread" is (max - min) / median over the windows of the reference contender (the plain kernel / the composition): the
run-to-run spread of this box.  The tool fails only where the fused layer is slower than the composition by more than that spread.  One
JSON line per measurement, appended to --out.
Usage: python tools/lora_dropout_bench.py [--out profiles/lora_dropout_bench.jsonl] [--iters 10] [--rounds 7] [--only kernel|layer]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import lora, ops, training  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.lora_bench import BF, RANKS, med, quantized, spread_of  # noqa: E402
from tools.train_linear_bench import DEV, PROBLEMS, emit  # noqa: E402

P = 0.1
SEED, OFFSET = 1234, (1 << 32) + 8


def bench_kernels(out, iters, rounds):
    thr = lora.dropout_threshold(P)
    drop = (thr, SEED, OFFSET)
    seen = set()
    for m, k, _ in PROBLEMS:
        for rank in RANKS:
            if (m, k, rank) in seen:
                continue
            seen.add((m, k, rank))
            g = torch.Generator(device=DEV).manual_seed(m + k + rank)
            x = torch.randn(m, k, device=DEV, dtype=BF, generator=g)
            down = torch.randn(rank, k, device=DEV, dtype=BF, generator=g) * 0.05
            g_t = torch.randn(m, rank, device=DEV, dtype=BF, generator=g) * 0.01
            gi = torch.randn(m, k, device=DEV, dtype=BF, generator=g)
            down_t = down.t().contiguous()
            ws = torch.empty(ops.lowrank_grad_workspace_bytes(m, k, rank) + 16, device=DEV, dtype=torch.uint8)
            pairs = {
                "lowrank_down": (lambda: ops.lowrank_down_dropout(x, down, *drop), lambda: ops.lowrank_down(x, down), 2 * m * k),
                "lowrank_grad": (lambda: ops.lowrank_grad_dropout(x, g_t, 1.0, *drop, out_t=True, workspace=ws),
                                 lambda: ops.lowrank_grad(x, g_t, 1.0, out_t=True, workspace=ws), 2 * m * k),
                # scale 0: gi keeps its values over the replays
                "lowrank_add": (lambda: ops.lowrank_add_dropout(g_t, down_t, gi, 0.0, *drop), lambda: ops.lowrank_add(g_t, down_t, gi, 0.0),
                                4 * m * k),
            }
            for name, (fused, plain, min_bytes) in pairs.items():
                r = race({"dropout": fused, "plain": plain}, 3 * iters, rounds)
                emit(out, dict(bench="dropout_kernel", kernel=name, tokens=m, k=k, rank=rank, dtype="bf16", p=P, dropout_us=med(r["dropout"]),
                               dropout_min_us=round(min(r["dropout"]), 2), plain_us=med(r["plain"]), plain_min_us=round(min(r["plain"]), 2),
                               spread=spread_of(r["plain"]), ratio=round(med(r["dropout"]) / med(r["plain"]), 3), min_bytes=min_bytes,
                               plain_bytes_per_s=round(min_bytes / (med(r["plain"]) * 1e-6)),
                               dropout_bytes_per_s=round(min_bytes / (med(r["dropout"]) * 1e-6)), device=torch.cuda.get_device_name(0)))
            del x, down, g_t, gi, down_t, ws


def eager_race(fns: dict, iters, rounds):
    """{name: [us per call of every round]}: eager calls between two device events, the contenders in alternation."""
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return times


def adapted(k, n, rank, dropout, up):
    model = torch.nn.Sequential(quantized(k, n, 1))
    assert sdnq_amd.add_lora(model, rank=rank, alpha=2 * rank, seed=3, dropout=dropout) == 1
    with torch.no_grad():
        model[0].lora_up.copy_(up)
    return model.train()


def bench_layer(out, iters, rounds):
    lost = []
    for m, k, n in PROBLEMS:
        for rank in RANKS:
            g = torch.Generator(device=DEV).manual_seed(m + k + n + rank)
            x = torch.randn(m, k, device=DEV, dtype=BF, generator=g).requires_grad_(True)
            dy = torch.randn(m, n, device=DEV, dtype=BF, generator=g) * 0.01
            up0 = torch.randn(n, rank, device=DEV, dtype=BF, generator=g) * 0.05
            fused, plain = adapted(k, n, rank, P, up0), adapted(k, n, rank, 0.0, up0)
            theirs = torch.nn.Sequential(quantized(k, n, 1))
            assert sdnq_amd.enable_input_grad(theirs) == 1
            fl, pl = fused[0], plain[0]
            down, up = fl.lora_down.detach().clone().requires_grad_(True), fl.lora_up.detach().clone().requires_grad_(True)
            scale = fl.lora_scale

            def fused_step():
                return torch.autograd.grad(fused(x), (x, fl.lora_down, fl.lora_up), dy)

            def plain_step():
                return torch.autograd.grad(plain(x), (x, pl.lora_down, pl.lora_up), dy)

            def composed_step():
                xd = torch.nn.functional.dropout(x, P, training=True)
                return torch.autograd.grad(theirs(x) + scale * ((xd @ down.t()) @ up.t()), (x, down, up), dy)
            r = eager_race({"fused": fused_step, "plain": plain_step, "composed": composed_step}, iters, rounds)
            spread = spread_of(r["composed"])
            line = dict(bench="dropout_layer", tokens=m, k=k, n=n, rank=rank, dtype="bf16", weights="int8_rowwise_w8a8", p=P, timing="eager",
                        fused_fwd_bwd_us=med(r["fused"]), fused_fwd_bwd_min_us=round(min(r["fused"]), 2),
                        plain_fwd_bwd_us=med(r["plain"]), plain_fwd_bwd_min_us=round(min(r["plain"]), 2),
                        composed_fwd_bwd_us=med(r["composed"]), composed_fwd_bwd_min_us=round(min(r["composed"]), 2), spread=spread,
                        ratio_to_plain=round(med(r["fused"]) / med(r["plain"]), 3),
                        ratio_to_composed=round(med(r["fused"]) / med(r["composed"]), 3), scratch_bytes=training.scratch_bytes(DEV),
                        device=torch.cuda.get_device_name(0))
            emit(out, line)
            if med(r["fused"]) > med(r["composed"]) * (1 + spread):
                lost.append(line)
            del fused, plain, theirs, fl, pl, x, dy, down, up, up0, r
            training.release_scratch()
            torch.cuda.empty_cache()
    return lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "lora_dropout_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("kernel", "layer"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_dropout_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    lost = []
    with open(a.out, "a") as f:
        if a.only in (None, "kernel"):
            bench_kernels(f, a.iters, a.rounds)
        if a.only in (None, "layer"):
            lost = bench_layer(f, a.iters, a.rounds)
    if lost:
        sys.exit("the fused dropout layer is slower than the torch composition beyond the run-to-run spread at: "
                 + ", ".join(f"{ln['tokens']}x{ln['k']}x{ln['n']} r{ln['rank']} ({ln['fused_fwd_bwd_us']} vs {ln['composed_fwd_bwd_us']} us)"
                             for ln in lost))


if __name__ == "__main__":
    main()
