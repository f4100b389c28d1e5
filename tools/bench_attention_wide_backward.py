#!/usr/bin/env python3
"""Kernel micro-benchmark (development aid): forward + backward of sdnq_hip_atten_with_backward at head dims above 128 (csrc/attention_wide.hip,
csrc/attention_wide_bwd.hip) against forward + backward of torch's SDPA in the same dtype, in one process.  Eager calls (an autograd backward
per call), REPS calls between two HIP events; the two are timed in turn for ROUNDS rounds.  Prints the median us per forward + backward and the
smallest / largest round of each.   Usage: python tools/bench_attention_wide_backward.py [bf16|f16]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import attention as A  # noqa: E402

dev = torch.device("cuda:0")
dt = torch.float16 if (len(sys.argv) > 1 and sys.argv[1] == "f16") else torch.bfloat16
# (batch, heads, q_len, kv_len, head_dim): the shapes of tools/bench_attention_wide.py
SHAPES = [(2, 8, 1024, 1024, 160), (2, 8, 4096, 77, 160), (1, 12, 4096, 4096, 256)]
REPS, ROUNDS = 10, 9


def step(fn, q, k, v, do):
    for x in (q, k, v):
        x.grad = None
    fn(q, k, v).backward(do)


def timed_us(fn, *t):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        step(fn, *t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


for (z, h, qn, kn, d) in SHAPES:
    q = torch.randn(z, h, qn, d, device=dev, dtype=dt, requires_grad=True)
    k = torch.randn(z, h, kn, d, device=dev, dtype=dt, requires_grad=True)
    v = torch.randn(z, h, kn, d, device=dev, dtype=dt, requires_grad=True)
    do = torch.randn(z, h, qn, d, device=dev, dtype=dt)
    fns = {"sdnq_hip_atten_with_backward": A.sdnq_hip_atten_with_backward, "torch sdpa": torch.nn.functional.scaled_dot_product_attention}
    times = {name: [] for name in fns}
    for fn in fns.values():  # warm up: code objects, allocator
        for _ in range(3):
            step(fn, q, k, v, do)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            times[name].append(timed_us(fn, q, k, v, do))
    print(f"Z={z} H={h} QN={qn:5d} KN={kn:5d} D={d:3d} {str(dt)[6:]}: " + "   ".join(
        f"{name} {statistics.median(t):9.1f} us (rounds {min(t):.1f} .. {max(t):.1f})" for name, t in times.items()), flush=True)
