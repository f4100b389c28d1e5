#!/usr/bin/env python3
"""DoRA on the quantized Linear adapters (sdnq_amd.lora, add_lora(use_dora=True)) on the eight problems of tools/train_linear_bench.py:
bf16, ranks 16 and 64, int8 row-wise and uint4 group-64 weights.

 (a) "norm": ops.dora_normsq (the squared row norms of W + s up down from the stored codes, one launch) against the composition a user
     has today: ``ops.dequant`` + ``torch.addmm(W, up, down, alpha=s)`` + ``.float().square().sum(1)``.  codes_bytes_per_s is the stored
     codes (scales and zero points included) over the kernel's time.  CONDITION: the tool fails where the kernel is slower than the
     composition beyond the composition's measured run-to-run spread.
 (b) "bwd": ops.dora_bwd (g = round(dY c) and q = sum_i dY (y - b), one pass) against ``dY * c`` plus
     ``(dY.float() * (y.float() - b)).sum(0)``.
 (c) "layer": forward + backward of the DoRA layer -- gradients for the input, both factors and the magnitude -- against
       plain     the same layer with plain LoRA: ratio_to_plain is the price of the feature;
       composed  the torch-autograd DoRA composition on the quantized layer under sdnq_amd.enable_input_grad (the norm from ops.dequant +
                 addmm, detached, as PEFT computes it).

hipGraph replays (a graph of `--iters` calls, `--rounds` rounds alternating the contenders), medians per call; "spread" is
(max - min) / median over the rounds of the reference contender.  Every case is recorded, a case that loses included.  One JSON line per
measurement, appended to --out.
Usage: python tools/dora_bench.py [--out profiles/dora_bench.jsonl] [--iters 10] [--rounds 7] [--only norm|bwd|layer] [--weights int8_rowwise|uint4_g64]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import linear, ops, training  # noqa: E402
from tools.input_grad_bench import FORMATS, race, stored_bytes  # noqa: E402
from tools.lora_bench import BF, RANKS, med, spread_of  # noqa: E402
from tools.train_linear_bench import DEV, PROBLEMS, emit  # noqa: E402

S = 1.5


def quantized(k, n, cfg, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=False, device=DEV, dtype=BF)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, device=DEV, dtype=BF, generator=g) * 0.05)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(**cfg))
    return layer


def bench_norm(out, iters, rounds, formats):
    lost = []
    for fmt in formats:
        seen = set()
        for _, k, n in PROBLEMS:
            if (n, k) in seen:
                continue
            seen.add((n, k))
            qw = linear._state(quantized(k, n, FORMATS[fmt])).qw
            for rank in RANKS:
                g = torch.Generator(device=DEV).manual_seed(n + k + rank)
                up = torch.randn(n, rank, device=DEV, dtype=BF, generator=g) * 0.05
                down = torch.randn(rank, k, device=DEV, dtype=BF, generator=g) * 0.05

                def composed():
                    return torch.addmm(ops.dequant(qw, BF, 0), up, down, alpha=S).float().square().sum(1)
                ref, got = composed().double(), ops.dora_normsq(qw, up, down, S).double()
                err = float(((got - ref).abs() / ref).max())  # (the composition rounds W + s up down to bf16: ~2^-8 per element)
                r = race({"kernel": lambda: ops.dora_normsq(qw, up, down, S), "composed": composed}, 3 * iters, rounds)
                spread, codes = spread_of(r["composed"]), stored_bytes(qw)
                line = dict(bench="dora_norm", weights=fmt, n=n, k=k, rank=rank, dtype="bf16", kernel_us=med(r["kernel"]),
                            kernel_min_us=round(min(r["kernel"]), 2), composed_us=med(r["composed"]), composed_min_us=round(min(r["composed"]), 2),
                            spread=spread, kernel_spread=spread_of(r["kernel"]), ratio=round(med(r["kernel"]) / med(r["composed"]), 3),
                            codes_bytes=codes, codes_bytes_per_s=round(codes / (med(r["kernel"]) * 1e-6)), max_rel_diff_to_composed=err,
                            device=torch.cuda.get_device_name(0))
                emit(out, line)
                if med(r["kernel"]) > med(r["composed"]) * (1 + spread):
                    lost.append(line)
            del qw
            torch.cuda.empty_cache()
    return lost


def bench_bwd(out, iters, rounds):
    seen = set()
    for m, _, n in PROBLEMS:
        if (m, n) in seen:
            continue
        seen.add((m, n))
        g = torch.Generator(device=DEV).manual_seed(m + n)
        dy = torch.randn(m, n, device=DEV, dtype=BF, generator=g) * 0.01
        y = torch.randn(m, n, device=DEV, dtype=BF, generator=g)
        b = torch.randn(n, device=DEV, dtype=BF, generator=g) * 0.1
        c = torch.rand(n, device=DEV, generator=g) + 0.5
        cb = c.to(BF)
        ws = torch.empty(ops.dora_bwd_workspace_bytes(m, n) + 16, device=DEV, dtype=torch.uint8)

        def composed():
            return dy * cb, (dy.float() * (y.float() - b)).sum(0)
        r = race({"kernel": lambda: ops.dora_bwd(dy, y, b, c, workspace=ws), "composed": composed}, 3 * iters, rounds)
        moved = 3 * m * n * 2  # dY and y read, g written
        emit(out, dict(bench="dora_bwd", tokens=m, n=n, dtype="bf16", kernel_us=med(r["kernel"]), kernel_min_us=round(min(r["kernel"]), 2),
                       composed_us=med(r["composed"]), composed_min_us=round(min(r["composed"]), 2), spread=spread_of(r["composed"]),
                       ratio=round(med(r["kernel"]) / med(r["composed"]), 3), min_bytes=moved,
                       kernel_bytes_per_s=round(moved / (med(r["kernel"]) * 1e-6)), device=torch.cuda.get_device_name(0)))
        del dy, y, ws
        torch.cuda.empty_cache()


def bench_layer(out, iters, rounds, formats):
    for fmt in formats:
        cfg = dict(FORMATS[fmt], use_quantized_matmul=True)
        for m, k, n in PROBLEMS:
            for rank in RANKS:
                g = torch.Generator(device=DEV).manual_seed(m + k + n + rank)
                x = torch.randn(m, k, device=DEV, dtype=BF, generator=g).requires_grad_(True)
                dy = torch.randn(m, n, device=DEV, dtype=BF, generator=g) * 0.01
                up0 = torch.randn(n, rank, device=DEV, dtype=BF, generator=g) * 0.05
                dora, plain, theirs = (torch.nn.Sequential(quantized(k, n, cfg)) for _ in range(3))
                assert sdnq_amd.add_lora(dora, rank=rank, alpha=2 * rank, seed=3, use_dora=True) == 1
                assert sdnq_amd.add_lora(plain, rank=rank, alpha=2 * rank, seed=3) == 1 and sdnq_amd.enable_input_grad(theirs) == 1
                dl, pl = dora[0], plain[0]
                with torch.no_grad():
                    dl.lora_up.copy_(up0), pl.lora_up.copy_(up0)
                down, up = dl.lora_down.detach().clone().requires_grad_(True), up0.clone().requires_grad_(True)
                mag = dl.lora_magnitude.detach().clone().requires_grad_(True)
                s, qw = dl.lora_scale, linear._state(theirs[0]).qw

                def dora_step():
                    return torch.autograd.grad(dora(x), (x, dl.lora_down, dl.lora_up, dl.lora_magnitude), dy)

                def plain_step():
                    return torch.autograd.grad(plain(x), (x, pl.lora_down, pl.lora_up), dy)

                def composed_step():
                    norm = torch.addmm(ops.dequant(qw, BF, 0), up.detach(), down.detach(), alpha=s).float().norm(dim=1)
                    cvec = (mag / norm).to(BF)
                    return torch.autograd.grad(cvec * (theirs(x) + s * ((x @ down.t()) @ up.t())), (x, down, up, mag), dy)
                r = race({"dora": dora_step, "plain": plain_step, "composed": composed_step}, iters, rounds)
                emit(out, dict(bench="dora_layer", weights=fmt, tokens=m, k=k, n=n, rank=rank, dtype="bf16", timing="hipGraph",
                               dora_fwd_bwd_us=med(r["dora"]), dora_fwd_bwd_min_us=round(min(r["dora"]), 2),
                               plain_fwd_bwd_us=med(r["plain"]), plain_fwd_bwd_min_us=round(min(r["plain"]), 2),
                               composed_fwd_bwd_us=med(r["composed"]), composed_fwd_bwd_min_us=round(min(r["composed"]), 2),
                               spread=spread_of(r["composed"]), ratio_to_plain=round(med(r["dora"]) / med(r["plain"]), 3),
                               ratio_to_composed=round(med(r["dora"]) / med(r["composed"]), 3), scratch_bytes=training.scratch_bytes(DEV),
                               device=torch.cuda.get_device_name(0)))
                del dora, plain, theirs, dl, pl, x, dy, down, up, mag, up0, r, qw
                training.release_scratch()
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dora_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("norm", "bwd", "layer"))
    ap.add_argument("--weights", choices=tuple(FORMATS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dora_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    formats = (a.weights,) if a.weights else tuple(FORMATS)
    lost = []
    with open(a.out, "a") as f:
        if a.only in (None, "norm"):
            lost = bench_norm(f, a.iters, a.rounds, formats)
        if a.only in (None, "bwd"):
            bench_bwd(f, a.iters, a.rounds)
        if a.only in (None, "layer"):
            bench_layer(f, a.iters, a.rounds, formats)
    if lost:
        sys.exit("ops.dora_normsq is slower than dequant + addmm + square-sum beyond the run-to-run spread at: "
                 + ", ".join(f"{ln['weights']} {ln['n']}x{ln['k']} r{ln['rank']} ({ln['kernel_us']} vs {ln['composed_us']} us)" for ln in lost))


if __name__ == "__main__":
    main()
