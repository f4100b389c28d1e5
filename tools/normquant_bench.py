#!/usr/bin/env python3
"""Normalisation + row quantization in one launch (ops.norm_rowquant, sdnq_amd.fuse_norms) against what runs without it.

 (a) "kernel": the torch norm (F.layer_norm, or the RMS composition in float32 with one rounding) + ``ops.rowquant`` -- two or more
     launches, y written and read back -- against the fused launch with the y store ("fused") and without it ("fused_noy"), bf16 rows
     with a bf16 affine weight (+ bias for LayerNorm), int8 codes.  alg_bytes: 2MK read + MK + 4M written (+ 2MK with y).
 (b) "block": the toy block of tests/test_fuse_norms_gpu.py at M x K -- LayerNorm -> three int8 w8a8 Linears (K -> K) on one input --
     through ``fuse_norms`` against the same block unfused, eager calls inside the graph as a model makes them.

hipGraph replays (a graph of `--iters` calls, `--rounds` rounds alternating the contenders), medians per call; "spread" is
(max - min) / median over the rounds of the unfused contender.  Every case is recorded, a case that loses included.  No threshold.
Usage: python tools/normquant_bench.py [--out profiles/normquant_bench.jsonl] [--iters 20] [--rounds 9] [--only kernel|block]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import linear, ops  # noqa: E402
from sdnq_amd.norms import fuse_norms, unfuse_norms  # noqa: E402
from tools.input_grad_bench import race  # noqa: E402
from tools.lora_bench import med, spread_of  # noqa: E402
from tools.train_linear_bench import DEV, emit  # noqa: E402

SHAPES = ((1024, 1280), (4096, 640), (1024, 2560), (4608, 3072), (4096, 4096))
EPS = 1e-5


def bench_kernel(out, iters, rounds):
    for m, k in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(m + k)
        x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16, generator=g)
        w = (1 + 0.1 * torch.randn(k, device=DEV, generator=g)).to(torch.bfloat16)
        b = (0.1 * torch.randn(k, device=DEV, generator=g)).to(torch.bfloat16)
        for norm in ("layer", "rms"):
            code, bias = (ops.NORM_LAYER, b) if norm == "layer" else (ops.NORM_RMS, None)

            def torch_norm():
                if norm == "layer":
                    return F.layer_norm(x, (k,), w, b, EPS)
                xf = x.float()
                return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS) * w).to(x.dtype)

            def unfused():
                return ops.rowquant(torch_norm(), ops.MM_I8, 0)

            def fused():
                return ops.norm_rowquant(x, code, EPS, w, bias, None, None, ops.MM_I8)

            def fused_noy():
                return ops.norm_rowquant(x, code, EPS, w, bias, None, None, ops.MM_I8, want_y=False)
            r = race({"unfused": unfused, "norm_only": torch_norm, "fused": fused, "fused_noy": fused_noy}, iters, rounds)
            nbytes = 3 * m * k + 4 * m
            emit(out, dict(bench="norm_rowquant", norm=norm, m=m, k=k, dtype="bf16", mm="int8", unfused_us=med(r["unfused"]),
                           torch_norm_us=med(r["norm_only"]), fused_us=med(r["fused"]), fused_noy_us=med(r["fused_noy"]),
                           spread=spread_of(r["unfused"]), fused_spread=spread_of(r["fused"]),
                           ratio=round(med(r["fused"]) / med(r["unfused"]), 3), ratio_noy=round(med(r["fused_noy"]) / med(r["unfused"]), 3),
                           alg_bytes_noy=nbytes, alg_bytes=nbytes + 2 * m * k, fused_TBps=round((nbytes + 2 * m * k) / med(r["fused"]) / 1e6, 3),
                           fused_noy_TBps=round(nbytes / med(r["fused_noy"]) / 1e6, 3), device=torch.cuda.get_device_name(0)))


class Block(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
        self.norm = torch.nn.LayerNorm(k).to(torch.bfloat16)
        self.q, self.k, self.v = (sdnq_amd.sdnq_quantize_layer(torch.nn.Linear(k, k).to(torch.bfloat16), cfg)[0] for _ in range(3))

    def forward(self, x):
        h = self.norm(x)
        return self.q(h), self.k(h), self.v(h)


@torch.no_grad()
def bench_block(out, iters, rounds):
    for m, k in SHAPES:
        torch.manual_seed(k)
        block = Block(k).to(DEV).eval()
        x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16)

        def step():
            linear.clear_activation_cache()
            return block(x)
        times = {}
        for name in ("unfused", "fused"):  # (the module is rewired between the two, so each is captured and replayed on its own)
            if name == "fused":
                fuse_norms(block)
            for _ in range(3):
                step()
            times[name] = race({name: step}, iters, rounds)[name]
        unfuse_norms(block)
        emit(out, dict(bench="norm_block", m=m, k=k, dtype="bf16", mm="int8", unfused_us=med(times["unfused"]), fused_us=med(times["fused"]),
                       spread=spread_of(times["unfused"]), fused_spread=spread_of(times["fused"]),
                       ratio=round(med(times["fused"]) / med(times["unfused"]), 3), device=torch.cuda.get_device_name(0)))
        del block
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "normquant_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--only", choices=("kernel", "block"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("normquant_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        if a.only != "block":
            bench_kernel(f, a.iters, a.rounds)
        if a.only != "kernel":
            bench_block(f, a.iters, a.rounds)


if __name__ == "__main__":
    main()
