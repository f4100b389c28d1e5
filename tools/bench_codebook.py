#!/usr/bin/env python3
"""Codebook layers (use_codebook=True) on the MI355X, one JSON line per measurement (results: profiles/codebook_bench.md):

  quantize  the HIP Lloyd-Max quantizer (sdnq_hip_quantize_codebook) per SDXL / FLUX Linear shape against the torch formulation of
            the same algorithm (sdnq_amd.quant_utils.quantize_codebook) on the same GPU;
  forward   uint4 codebook Linear layers against plain uint4 layers of the same shape, int8 matmul: cached mode, per-call mode
            (SDNQ_HIP_CACHE_WEIGHTS=0: re-quantization, or the gemm_w4 route for few rows, on every call) and float mode;
  gather    embedding rows of a uint4 codebook table against a plain uint4 table.

Median microseconds over hipEvent-timed repeats after warm-up.

    python tools/bench_codebook.py [--repeats 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sdnq_amd  # noqa: E402
import sdnq_amd.linear as L  # noqa: E402
from sdnq_amd import _lib, ops  # noqa: E402
from sdnq_amd.quant_utils import quantize_codebook  # noqa: E402

SHAPES = {"sdxl_attn": (1280, 1280), "sdxl_ff_up": (10240, 1280), "sdxl_ff_down": (1280, 5120), "flux_qkv": (9216, 3072),
          "flux_mlp_up": (12288, 3072), "flux_mlp_down": (3072, 12288)}  # (N, K)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return times[len(times) // 2]


def layer(n, k, codebook, dev, mm=True):
    torch.manual_seed(0)
    lin = torch.nn.Linear(k, n, device=dev, dtype=torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=codebook, use_quantized_matmul=mm)
    return sdnq_amd.sdnq_quantize_layer(lin, cfg)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []

    def emit(**kw):
        kw["lib"] = _lib.source_hash() if hasattr(_lib, "source_hash") else None
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    for name, (n, k) in SHAPES.items():
        w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
        hip = timed(lambda: ops.quantize_codebook(w, "uint4", 256), 1, 3)
        ref = timed(lambda: quantize_codebook(w.view(n, k // 256, 256), -1, "uint4"), 1, 3)
        emit(kind="quantize", shape=name, n=n, k=k, weights_dtype="uint4", group=256, hip_us=hip, torch_gpu_us=ref, speedup=ref / hip)
    with torch.no_grad():
        for name, (n, k) in SHAPES.items():
            for m in (1, 16, 64, 1024, 4096):
                x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
                row = dict(kind="forward", shape=name, n=n, k=k, m=m)
                for tag, cb in (("plain", False), ("codebook", True)):
                    lay = layer(n, k, cb, dev)
                    L.CACHE_WEIGHTS = True
                    lay.__dict__.pop("_sdnq_hip_state", None)
                    row[f"{tag}_cached_us"] = timed(lambda: lay(x), args.warmup, args.repeats)
                    L.CACHE_WEIGHTS = False
                    lay.__dict__.pop("_sdnq_hip_state", None)
                    row[f"{tag}_percall_us"] = timed(lambda: lay(x), args.warmup, args.repeats)
                    L.CACHE_WEIGHTS = True
                    flt = layer(n, k, cb, dev, mm=False)
                    row[f"{tag}_float_us"] = timed(lambda: flt(x), args.warmup, args.repeats)
                    del lay, flt
                emit(**row)
        for V, D in ((32128, 4096), (128256, 4096)):
            row = dict(kind="gather", V=V, D=D)
            for tag, cb in (("plain", False), ("codebook", True)):
                torch.manual_seed(0)
                emb = torch.nn.Embedding(V, D, device=dev, dtype=torch.bfloat16)
                q = sdnq_amd.sdnq_quantize_layer(emb, sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=cb, quant_embedding=True))[0]
                for nids in (1, 8192):
                    ids = torch.randint(0, V, (nids,), device=dev)
                    row[f"{tag}_{nids}_us"] = timed(lambda: q(ids), args.warmup, args.repeats)
                del q, emb
            emit(**row)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
