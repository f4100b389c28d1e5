#!/usr/bin/env python3
"""The int8 training Linear (sdnq_amd.training) on training-sized problems: tokens 4096 and 16384 at the SDXL and FLUX projection widths.

 (a) "colquant": sdnq_hip_colquant_t against the same arithmetic composed from torch ops on the same GPU -- abs().amax(0), div, round,
     clamp, to(int8), t().contiguous() in float32 -- once with the float32 upcast of the 16-bit input inside the timed region (what the
     reference does) and once on an input that is float32 already (the composition alone).  bytes_per_s is the algorithm's minimum for
     a 16-bit input, 5 B per element (two reads, one write of codes), over the measured time.
 (b) "linear": forward + backward of both variants against torch.nn.functional.linear forward + backward in bf16, and the split of
     the plain variant over its nine launches' operators, each timed alone.

Everything is timed as hipGraph replays (no host launch cost in the numbers): a graph of `--iters` calls, device events around one
replay, `--rounds` rounds alternating the contenders; median and min per call.  One JSON line per measurement, appended to --out.
Usage: python tools/train_linear_bench.py [--out profiles/train_linear_bench.jsonl] [--iters 10] [--rounds 7] [--only colquant|linear]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import ops, training  # noqa: E402
from sdnq_amd._lib import MM_I8  # noqa: E402

DEV = torch.device("cuda:0")
# (tokens, K, N): SDXL attention / feed-forward projections and FLUX.1-dev's
PROBLEMS = [(4096, 640, 640), (4096, 640, 5120), (4096, 1280, 1280), (4096, 3072, 3072), (16384, 640, 640), (16384, 1280, 5120),
            (16384, 3072, 3072), (16384, 3072, 12288)]


def capture(fn, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def race(fns: dict, iters, rounds):
    """{name: (median us, min us)} per call of each fn, the graphs replayed in alternation."""
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
    return {k: (round(statistics.median(v), 2), round(min(v), 2)) for k, v in times.items()}


def torch_colquant(x32):
    scale = x32.abs().amax(0, keepdim=True) / 127
    return torch.div(x32, scale).round_().clamp_(-128, 127).to(torch.int8).t().contiguous(), scale


def bench_colquant(out, iters, rounds):
    """Returns the lines at which colquant_t was NOT faster than the torch composition on a float32 input (the condition of (a))."""
    seen, lost = set(), []
    for m, k, n in PROBLEMS:
        for what, (r, c) in (("x", (m, k)), ("dy", (m, n)), ("w", (n, k))):
            if (r, c) in seen:
                continue
            seen.add((r, c))
            g = torch.Generator(device=DEV).manual_seed(r + c)
            x = torch.randn(r, c, device=DEV, dtype=torch.bfloat16, generator=g)
            x32 = x.float()
            q, s = torch_colquant(x32)
            mine = ops.colquant_t(x)
            # same arithmetic, not always the same bits: torch's GPU kernel divides by the scalar 127 as a multiply by its reciprocal, so a
            # scale may sit one ulp off and move a code that lies on a rounding boundary (the tests hold colquant_t to the reference's bits)
            off = (mine[0][:, :r].int() - q.int()).abs()
            srel = ((mine[1].reshape(-1) - s.reshape(-1)).abs() / s.reshape(-1)).max().item()
            assert off.max().item() <= 1 and off.float().mean().item() < 1e-3 and srel <= 2.0 ** -22, "colquant_t differs from the torch composition"
            res = race({"hip": lambda: ops.colquant_t(x, want_colsum=True), "torch_upcast": lambda: torch_colquant(x.float()),
                        "torch_f32": lambda: torch_colquant(x32)}, 3 * iters, rounds)
            hip = res["hip"][0]
            line = dict(bench="colquant", operand=what, rows=r, cols=c, dtype="bf16", colquant_t_us=hip, colquant_t_min_us=res["hip"][1],
                        torch_ops_with_upcast_us=res["torch_upcast"][0], torch_ops_f32_input_us=res["torch_f32"][0],
                        torch_ops_f32_input_min_us=res["torch_f32"][1], speedup_vs_f32_input=round(res["torch_f32"][0] / hip, 2),
                        codes_off_by_one=int(off.sum().item()), min_bytes=5 * r * c, bytes_per_s=round(5 * r * c / (hip * 1e-6)), device=torch.cuda.get_device_name(0))
            emit(out, line)
            if hip >= res["torch_f32"][0]:
                lost.append(line)
            del x, x32, q, s, mine, off
    return lost


def bench_linear(out, iters, rounds):
    for m, k, n in PROBLEMS:
        g = torch.Generator(device=DEV).manual_seed(m + k + n)
        x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16, generator=g).requires_grad_(True)
        w = (torch.randn(n, k, device=DEV, dtype=torch.bfloat16, generator=g) * 0.05).requires_grad_(True)
        b = torch.zeros(n, device=DEV, dtype=torch.bfloat16).requires_grad_(True)
        dy = torch.randn(m, n, device=DEV, dtype=torch.bfloat16, generator=g) * 0.01

        def step(fn):
            return lambda: torch.autograd.grad(fn(x, w, b), (x, w, b), dy)
        res = race({"plain": step(training.int8_matmul_dynamic_with_backward), "ckpt": step(training.int8_matmul_dynamic_with_backward_ckpt),
                    "bf16": step(torch.nn.functional.linear)}, iters, rounds)
        xd, wd = x.detach(), w.detach()
        xq, xs, _, _ = ops.rowquant(xd, MM_I8)
        wq, ws, _, _ = ops.rowquant(wd, MM_I8)
        gq, gs, _, _ = ops.rowquant(dy, MM_I8)
        wq_t, wsc, _ = ops.colquant_t(wd)
        gq_t, gs_t, _ = ops.colquant_t(dy)
        xq_t, xsc, _ = ops.colquant_t(xd)
        split = race({
            "rowquant_x": lambda: ops.rowquant(xd, MM_I8), "rowquant_w": lambda: ops.rowquant(wd, MM_I8),
            "mm_y": lambda: ops.scaled_mm(MM_I8, xq, wq, xs, ws, b.detach(), torch.bfloat16),
            "rowquant_dy": lambda: ops.rowquant(dy, MM_I8), "colquant_w": lambda: ops.colquant_t(wd),
            "mm_grad_input": lambda: ops.scaled_mm(MM_I8, gq, wq_t, gs, wsc, None, torch.bfloat16),
            "colquant_dy_colsum": lambda: ops.colquant_t(dy, want_colsum=True), "colquant_x": lambda: ops.colquant_t(xd),
            "mm_grad_weight": lambda: ops.scaled_mm(MM_I8, gq_t, xq_t, gs_t, xsc, None, torch.bfloat16),
        }, iters, rounds)
        line = dict(bench="linear", tokens=m, k=k, n=n, dtype="bf16", int8_fwd_bwd_us=res["plain"][0], int8_ckpt_fwd_bwd_us=res["ckpt"][0],
                    torch_bf16_fwd_bwd_us=res["bf16"][0], int8_min_us=res["plain"][1], torch_bf16_min_us=res["bf16"][1],
                    ratio=round(res["plain"][0] / res["bf16"][0], 3), split_us={key: v[0] for key, v in split.items()},
                    split_sum_us=round(sum(v[0] for v in split.values()), 1), device=torch.cuda.get_device_name(0))
        emit(out, line)
        del x, w, b, dy, xq, wq, gq, wq_t, gq_t, xq_t


def emit(out, line):
    print(json.dumps(line), flush=True)
    out.write(json.dumps(line) + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "train_linear_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("colquant", "linear"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_linear_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        lost = bench_colquant(f, a.iters, a.rounds) if a.only != "linear" else []
        if a.only != "colquant":
            bench_linear(f, a.iters, a.rounds)
    if lost:
        sys.exit("colquant_t is not faster than the torch composition at: " + ", ".join(f"{ln['rows']}x{ln['cols']}" for ln in lost))


if __name__ == "__main__":
    main()
