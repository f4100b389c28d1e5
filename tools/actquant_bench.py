#!/usr/bin/env python3
"""Activation + gate product + row quantization in one launch (ops.act_rowquant, sdnq_amd.fuse_activations) against what runs without
it: torch's activation (+ ``chunk`` / ``mul``) followed by ``ops.rowquant`` -- three or four launches, the [M][N] product written and
read back -- at the feed-forward shapes of SDXL (GEGLU on one [M][2N] projection output), FLUX (GELU(tanh)) and an LLM block (SwiGLU
on two tensors); bf16 rows, int8 codes, the fused launch with the y store ("fused") and without it ("fused_noy").

alg_bytes: 2MN per operand read + MN + 4M written (+ 2MN with y).  hipGraph replays (a graph of `--iters` calls, `--rounds` rounds
alternating the contenders), medians per call; "spread" is (max - min) / median over the rounds of the composition.  Every case is
recorded, a case that loses included ("loses": the fused median is above the composition's by more than the larger spread).
Usage: python tools/actquant_bench.py [--out profiles/actquant_bench.jsonl] [--iters 20] [--rounds 9]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import ops  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.lora_bench import med, spread_of  # noqa: E402
from tools.train_linear_bench import DEV, emit  # noqa: E402

# (name, act, layout, M, N)
CASES = (("geglu", "gelu", "halves", 4096, 2560), ("geglu", "gelu", "halves", 1024, 5120),
         ("gelu_tanh", "gelu_tanh", "ungated", 4608, 12288), ("swiglu", "silu", "two", 2048, 14336))
ACTS = {"gelu": (ops.ACT_GELU, F.gelu), "gelu_tanh": (ops.ACT_GELU_TANH, lambda t: F.gelu(t, approximate="tanh")), "silu": (ops.ACT_SILU, F.silu)}


def bench(out, iters, rounds):
    lost = []
    for name, act, layout, m, n in CASES:
        g = torch.Generator(device=DEV).manual_seed(m + n)
        code, torch_act = ACTS[act]
        h = torch.randn(m, 2 * n if layout == "halves" else n, device=DEV, dtype=torch.bfloat16, generator=g)
        if layout == "halves":
            a, b = h[:, n:], h[:, :n]
        else:
            a, b = h, (torch.randn(m, n, device=DEV, dtype=torch.bfloat16, generator=g) if layout == "two" else None)

        def torch_only():
            if layout == "halves":  # as the module writes it
                value, gate = h.chunk(2, dim=-1)
                return value * torch_act(gate)
            return torch_act(a) if b is None else torch_act(a) * b

        def composed():
            return ops.rowquant(torch_only(), ops.MM_I8, 0)

        def fused():
            return ops.act_rowquant(a, b, code, ops.MM_I8)

        def fused_noy():
            return ops.act_rowquant(a, b, code, ops.MM_I8, want_y=False)
        r = race({"composed": composed, "torch_only": torch_only, "fused": fused, "fused_noy": fused_noy}, iters, rounds)
        nbytes = (2 if b is None else 4) * m * n + m * n + 4 * m
        slack = max(spread_of(r["composed"]), spread_of(r["fused"]))
        rec = dict(bench="act_rowquant", case=name, act=act, layout=layout, m=m, n=n, dtype="bf16", mm="int8", composed_us=med(r["composed"]),
                   torch_act_us=med(r["torch_only"]), fused_us=med(r["fused"]), fused_noy_us=med(r["fused_noy"]),
                   spread=spread_of(r["composed"]), fused_spread=spread_of(r["fused"]),
                   ratio=round(med(r["fused"]) / med(r["composed"]), 3), ratio_noy=round(med(r["fused_noy"]) / med(r["composed"]), 3),
                   alg_bytes_noy=nbytes, alg_bytes=nbytes + 2 * m * n, fused_TBps=round((nbytes + 2 * m * n) / med(r["fused"]) / 1e6, 3),
                   fused_noy_TBps=round(nbytes / med(r["fused_noy"]) / 1e6, 3), device=torch.cuda.get_device_name(0))
        rec["loses"] = [k for k in ("fused", "fused_noy") if med(r[k]) > med(r["composed"]) * (1 + slack)]
        lost += [(name, m, n, k) for k in rec["loses"]]
        emit(out, rec)
    return lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "actquant_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("actquant_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        lost = bench(f, a.iters, a.rounds)
    print("cases the fused launch loses beyond the spread:", lost or "none")


if __name__ == "__main__":
    main()
