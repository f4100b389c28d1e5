#!/usr/bin/env python3
"""Gather-dequantize of quantized embeddings (SDNQEmbedding.forward -> sdnq_hip_embedding) against
  (a) F.embedding on a bfloat16 table of the same shape, and
  (b) "dequantize the whole table, then index" (what a user without the fused kernel falls back to).

One JSON line per (table shape, n_ids, format): median microseconds over hipEvent-timed repeats after warm-up, the bytes the
fused kernel moves (gathered rows of codes / scales / zero points / svd_up, svd_down once, ids, the output), the resulting GB/s,
the two baselines' times and the library's source hash.

    python tools/bench_embedding.py [--repeats 30] [--warmup 5] [--shapes t5,llama3,gemma] [--ns 1,512,8192]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import sdnq_amd  # noqa: E402
from sdnq_amd import _lib  # noqa: E402

SHAPES = {"llama3": (128256, 4096), "gemma": (262144, 3840), "t5": (32128, 4096)}
FORMATS = {
    "int8": dict(weights_dtype="int8", group_size=-1),
    "int4_g32": dict(weights_dtype="int4", group_size=32),
    "uint4": dict(weights_dtype="uint4"),
    "fp8": dict(weights_dtype="float8_e4m3fn", group_size=-1),
    "int4_had256": dict(weights_dtype="int4", use_hadamard=True, hadamard_group_size=256),
    "int8_svd32": dict(weights_dtype="int8", group_size=-1, use_svd=True, svd_rank=32),
}


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


def nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="t5,llama3,gemma")
    ap.add_argument("--ns", default="1,512,8192")
    ap.add_argument("--formats", default=",".join(FORMATS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    srchash = open(_lib.LIB_PATH + ".srchash").read().strip()[:12]
    ns = [int(n) for n in args.ns.split(",")]
    with torch.no_grad():
        for shape in args.shapes.split(","):
            V, D = SHAPES[shape]
            torch.manual_seed(0)
            table = (torch.randn(V, D, device=dev) * 0.02).to(torch.bfloat16)
            ids_by_n = {n: torch.randint(0, V, (n,), device=dev) for n in ns}
            base_a = {n: timed(lambda n=n: F.embedding(ids_by_n[n], table), args.warmup, args.repeats) for n in ns}
            for fmt in args.formats.split(","):
                emb = torch.nn.Embedding.from_pretrained(table.clone(), freeze=True)
                layer, _ = sdnq_amd.sdnq_quantize_layer(emb, sdnq_amd.SDNQConfig(quant_embedding=True, **FORMATS[fmt]))
                dq = layer.sdnq_dequantizer
                row_bytes = (nbytes(layer.weight) + nbytes(layer.scale) + nbytes(layer.zero_point) + nbytes(layer.svd_up)) / V
                for n in ns:
                    ids = ids_by_n[n]
                    us = timed(lambda: layer(ids), args.warmup, args.repeats)
                    reps_b = max(3, args.repeats // 5)  # whole-table dequantize: milliseconds per call
                    us_b = timed(lambda: dq(layer.weight, layer.scale, zero_point=layer.zero_point, svd_up=layer.svd_up,
                                            svd_down=layer.svd_down)[ids], 2, reps_b)
                    moved = int(n * row_bytes + nbytes(layer.svd_down) + nbytes(ids) + n * D * 2)
                    print(json.dumps(dict(case=f"{shape}_{fmt}_n{n}", V=V, D=D, n_ids=n, format=fmt, us=round(us, 2), bytes=moved,
                                          gbps=round(moved / us / 1e3, 1), us_f_embedding_bf16=round(base_a[n], 2),
                                          us_dequant_then_index=round(us_b, 1), srchash=srchash)), flush=True)
                del layer, emb
                torch.cuda.empty_cache()
            del table


if __name__ == "__main__":
    main()
