#!/usr/bin/env python3
"""The fused producers for rotated consumers (``hadamard_group=256`` of ops.norm_rowquant / ops.act_rowquant) against what runs
without them: the plain producer writing only y (``mm=None``) followed by ``ops.rowquant(y, mm, 256)`` -- two launches, y read back by
the rotated row quantizer.  bf16 rows, int8 codes, group 256, at the FLUX shapes (adaLN LayerNorm and RMSNorm 4608 x 3072, GELU(tanh)
4608 x 12288) and SDXL's GEGLU (4096 x 2560 from a 4096 x 5120 projection output).

alg_bytes: 2MK per operand read + 2MK (y) + MK + 4M written.  hipGraph replays (a graph of `--iters` calls, `--rounds` rounds
alternating the contenders), medians per call; "spread" is (max - min) / median over the rounds.  Every case is recorded, a case that
loses included ("loses": the fused median is above the composition's by more than the larger spread).
Usage: python tools/producer_hadamard_bench.py [--out profiles/producer_hadamard_bench.jsonl] [--iters 20] [--rounds 9]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import ops  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.lora_bench import med, spread_of  # noqa: E402
from tools.train_linear_bench import DEV, emit  # noqa: E402

GROUP = 256
# (name, producer, M, K)
CASES = (("adaln_layernorm", "norm", 4608, 3072), ("rmsnorm", "norm", 4608, 3072), ("gelu_tanh", "act", 4608, 12288),
         ("geglu", "act", 4096, 2560))


def contenders(name, m, k):
    """(producer(mm, hadamard_group) -> (y, xq, xs), operands read per element)"""
    g = torch.Generator(device=DEV).manual_seed(m + k)
    rand = lambda *shape: torch.randn(*shape, device=DEV, dtype=torch.bfloat16, generator=g)  # noqa: E731
    if name == "adaln_layernorm":
        x, scale, shift = rand(m, k), 0.3 * rand(1, k), 0.5 * rand(1, k)
        return lambda mm, had: ops.norm_rowquant(x, ops.NORM_LAYER, 1e-6, None, None, scale, shift, mm, hadamard_group=had), 1
    if name == "rmsnorm":
        x, w = rand(m, k), 1 + 0.1 * rand(k)
        return lambda mm, had: ops.norm_rowquant(x, ops.NORM_RMS, 1e-6, w, None, None, None, mm, hadamard_group=had), 1
    if name == "gelu_tanh":
        a = rand(m, k)
        return lambda mm, had: ops.act_rowquant(a, None, ops.ACT_GELU_TANH, mm, hadamard_group=had), 1
    h = rand(m, 2 * k)  # geglu: the two halves of one projection output
    return lambda mm, had: ops.act_rowquant(h[:, k:], h[:, :k], ops.ACT_GELU, mm, hadamard_group=had), 2


def bench(out, iters, rounds):
    lost = []
    for name, producer, m, k in CASES:
        run, operands = contenders(name, m, k)

        def composed():
            return ops.rowquant(run(None, 0)[0], ops.MM_I8, GROUP)

        def fused():
            return run(ops.MM_I8, GROUP)
        y, xq, xs = fused()
        rq, rs, _, _ = composed()
        assert torch.equal(xq, rq) and torch.equal(xs, rs) and torch.equal(y, run(None, 0)[0]), f"{name}: the contenders disagree"
        r = race({"composed": composed, "fused": fused}, iters, rounds)
        nbytes = (2 * operands + 2 + 1) * m * k + 4 * m
        slack = max(spread_of(r["composed"]), spread_of(r["fused"]))
        rec = dict(bench="producer_hadamard", case=name, producer=producer, m=m, k=k, dtype="bf16", mm="int8", hadamard_group=GROUP,
                   composed_us=med(r["composed"]), fused_us=med(r["fused"]), spread=spread_of(r["composed"]), fused_spread=spread_of(r["fused"]),
                   ratio=round(med(r["fused"]) / med(r["composed"]), 3), alg_bytes=nbytes, fused_TBps=round(nbytes / med(r["fused"]) / 1e6, 3),
                   loses=med(r["fused"]) > med(r["composed"]) * (1 + slack), device=torch.cuda.get_device_name(0))
        if rec["loses"]:
            lost.append((name, m, k))
        emit(out, rec)
    return lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "producer_hadamard_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("producer_hadamard_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        lost = bench(f, a.iters, a.rounds)
    print("cases the fused launch loses beyond the spread:", lost or "none")


if __name__ == "__main__":
    main()
