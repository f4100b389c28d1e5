#!/usr/bin/env python3
"""The backward of a frozen quantized Linear (sdnq_amd.training.QuantizedLinearInputGrad) on training-sized problems: tokens 4096 and 16384
at the SDXL and FLUX projection widths of tools/train_linear_bench.py, bf16, int8 row-wise and uint4 group-64 weights.  Per problem:

 (a) "dequant_t_us": sdnq_hip_dequant_t alone; bytes = stored codes + scales (+ zero points) read + the [K][N] bf16 operand written, and
     the resulting bytes_per_s;
 (b) "backward_us": the whole backward -- ops.weight_t into the scratch buffer + the float GEMM (ops.linear_float);
 (c) "mm_resident_us": torch.mm(dY, W_float) on a RESIDENT bf16 copy of the weight: the baseline, which spends the memory this feature saves;
 (d) "composed_us": ops.dequant + .t().contiguous() + torch.mm: what a user could assemble without the new kernel.

Everything is timed as hipGraph replays (no host launch cost in the numbers): a graph of `--iters` calls, device events around one replay,
`--rounds` rounds alternating the contenders; median and min per call.  "spread" is (max - min) / median over (d)'s own windows, the
run-to-run spread of this box; the tool fails only where (b) is slower than (d) by more than that.  One JSON line per problem, appended
to --out.
Usage: python tools/input_grad_bench.py [--out profiles/input_grad_bench.jsonl] [--iters 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import linear, ops, training  # noqa: E402
from tools.train_linear_bench import DEV, PROBLEMS, capture, emit  # noqa: E402

FORMATS = {"int8_rowwise": dict(weights_dtype="int8", group_size=-1), "uint4_g64": dict(weights_dtype="uint4", group_size=64)}


def race(fns: dict, iters, rounds):
    """{name: [us per call of every round]}, the graphs replayed in alternation."""
    graphs = {k: capture(f, iters) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return times


def stored_bytes(qw):
    return sum(t.numel() * t.element_size() for t in qw.keep[:3] if t is not None)


def bench(out, iters, rounds):
    lost = []
    for fmt, cfg in FORMATS.items():
        for m, k, n in PROBLEMS:
            g = torch.Generator(device=DEV).manual_seed(m + k + n)
            lin = torch.nn.Linear(k, n, bias=False, device=DEV, dtype=torch.bfloat16)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(n, k, device=DEV, dtype=torch.bfloat16, generator=g) * 0.05)
            layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(**cfg))
            qw = linear._state(layer).qw
            dy = torch.randn(m, n, device=DEV, dtype=torch.bfloat16, generator=g) * 0.01
            w_float = ops.dequant(qw, torch.bfloat16, 0)                      # [N, K], resident for (c)
            scratch = (sdnq_amd.scratch.take(DEV, "input-gradient scratch", 2 * n * k, "operand")[0].view(torch.bfloat16), None)

            def backward():
                return ops.linear_float(dy, ops.weight_t(qw, torch.bfloat16, 0, scratch), None)

            def composed():
                return torch.mm(dy, ops.dequant(qw, torch.bfloat16, 0).t().contiguous().t())
            ref = torch.mm(dy, w_float).float()
            for name, got in (("backward", backward()), ("composed", composed())):
                err = float((got.float() - ref).abs().max() / ref.abs().max())
                assert err <= 2 * 2.0 ** -8, (name, fmt, m, k, n, err)                # one bf16 rounding of another summation order
            t = race({"dequant_t": lambda: ops.dequant_t(qw, torch.bfloat16, out=scratch[0][:n * k]), "backward": backward,
                      "mm_resident": lambda: torch.mm(dy, w_float), "composed": composed}, iters, rounds)
            med = {key: round(statistics.median(v), 2) for key, v in t.items()}
            spread = round((max(t["composed"]) - min(t["composed"])) / statistics.median(t["composed"]), 4)
            nbytes = stored_bytes(qw) + 2 * n * k
            line = dict(bench="input_grad", format=fmt, tokens=m, k=k, n=n, dtype="bf16", dequant_t_us=med["dequant_t"],
                        dequant_t_min_us=round(min(t["dequant_t"]), 2), dequant_t_bytes=nbytes,
                        dequant_t_bytes_per_s=round(nbytes / (med["dequant_t"] * 1e-6)), backward_us=med["backward"],
                        backward_min_us=round(min(t["backward"]), 2), mm_resident_us=med["mm_resident"], composed_us=med["composed"],
                        composed_min_us=round(min(t["composed"]), 2), spread=spread, backward_vs_resident=round(med["backward"] / med["mm_resident"], 3),
                        backward_vs_composed=round(med["backward"] / med["composed"], 3), scratch_bytes=2 * n * k,
                        resident_float_bytes=2 * n * k, device=torch.cuda.get_device_name(0))
            emit(out, line)
            if med["backward"] > med["composed"] * (1 + spread):
                lost.append(line)
            del lin, layer, qw, dy, w_float, scratch, ref
            training.release_scratch()
    return lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "input_grad_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("input_grad_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        lost = bench(f, a.iters, a.rounds)
    if lost:
        sys.exit("the backward is slower than dequant + transpose + torch.mm beyond the run-to-run spread at: "
                 + ", ".join(f"{ln['format']} {ln['tokens']}x{ln['n']}x{ln['k']}" for ln in lost))


if __name__ == "__main__":
    main()
