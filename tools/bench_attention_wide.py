#!/usr/bin/env python3
"""Kernel micro-benchmark (development aid): sdnq_hip_atten at head dims above 128 (csrc/attention_wide.hip) against torch's SDPA in the same
dtype.  Every call sequence is captured into a hipGraph once; the two graphs are replayed in turn for ROUNDS rounds and timed with HIP
events.  Prints the median us per call and the smallest / largest round of each.   Usage: python tools/bench_attention_wide.py [bf16|f16]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import attention as A  # noqa: E402

dev = torch.device("cuda:0")
dt = torch.float16 if (len(sys.argv) > 1 and sys.argv[1] == "f16") else torch.bfloat16
# (batch, heads, q_len, kv_len, head_dim): the deepest SD 1.5 blocks at 512 px with batch 2 (self- and cross-attention, head dim 160), 12 heads of 256
SHAPES = [(2, 8, 1024, 1024, 160), (2, 8, 4096, 77, 160), (1, 12, 4096, 4096, 256)]
REPS, ROUNDS = 10, 15


def captured(fn, s):
    fn()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(REPS):
            fn()
    g.replay()
    s.synchronize()
    return g


def replay_us(g, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(3):
        g.replay()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / (3 * REPS) * 1e3


for (z, h, qn, kn, d) in SHAPES:
    q = torch.randn(z, h, qn, d, device=dev, dtype=dt)
    k = torch.randn(z, h, kn, d, device=dev, dtype=dt)
    v = torch.randn(z, h, kn, d, device=dev, dtype=dt)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        graphs = {"sdnq_hip_atten": captured(lambda: A.sdnq_hip_atten(q, k, v), s),
                  "torch sdpa": captured(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), s)}
        times = {name: [] for name in graphs}
        for _ in range(ROUNDS):
            for name, g in graphs.items():
                times[name].append(replay_us(g, s))
    ops = 4.0 * z * h * qn * kn * d
    print(f"Z={z} H={h} QN={qn:5d} KN={kn:5d} D={d:3d} {str(dt)[6:]}: " + "   ".join(
        f"{name} {statistics.median(t):8.1f} us (rounds {min(t):.1f} .. {max(t):.1f}, {ops / statistics.median(t) / 1e6:6.1f} TOP/s)" for name, t in times.items()), flush=True)
