#!/usr/bin/env python3
"""Merging a low-rank adapter into the stored codes (ops.merge_lowrank, sdnq_amd.merge_lora) on the weight shapes of the eight problems
of tools/train_linear_bench.py: bf16 factors, ranks 16 and 64, int8 row-wise weights (the kernel's two-sweep form) and uint4 group-64
weights (one sweep).

 (a) "merge": ops.merge_lowrank (codes -> codes, one launch) against the composition a user has today, both in the same run on the same
     build: ``ops.dequant`` to float32 + ``torch.addmm(W, up, down, alpha=s)`` + ``ops.quantize_weight``.  codes_bytes_per_s is the stored
     codes (scales and zero points included) over the kernel's time.  The outputs of the two are compared: mismatch counts the code bytes
     that differ (the composition's addmm sums in another order and does not fuse the multiply-add, so a few codes on a rounding edge may).
     CONDITION: the tool fails where the fused kernel is slower than the composition beyond the composition's measured run-to-run
     spread; such a case belongs to the composition route of sdnq_amd.lora._merge_layer.
 (b) "sdxl": rank-16 adapters on every Linear of the SDXL UNet step (sdnq_amd.shapes.sdxl_unet_linears, int8 row-wise), merged by
     ``sdnq_amd.merge_lora`` end to end -- host work included -- on the fused route and with every layer forced through the composition.
     One wall-clock measurement each (a merge cannot be replayed: it consumes the adapters), after a warm-up merge of a small model.

(a): hipGraph replays (a graph of `--iters` calls, `--rounds` rounds alternating the contenders), medians per call; "spread" is
(max - min) / median over the rounds of the composition.  Every case is recorded, a case that loses included.  One JSON line per measurement,
appended to --out.
Usage: python tools/merge_bench.py [--out profiles/merge_bench.jsonl] [--iters 10] [--rounds 7] [--only merge|sdxl] [--weights int8_rowwise|uint4_g64]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdnq_amd  # noqa: E402
from sdnq_amd import linear, lora, ops, shapes  # noqa: E402
from tools.dora_bench import quantized  # noqa: E402
from tools.input_grad_bench import FORMATS, race, stored_bytes  # noqa: E402
from tools.lora_bench import BF, RANKS, med, spread_of  # noqa: E402
from tools.train_linear_bench import DEV, PROBLEMS, emit  # noqa: E402

S = 1.5


def bench_merge(out, iters, rounds, formats):
    lost = []
    for fmt in formats:
        wdt = FORMATS[fmt]["weights_dtype"]
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
                upf, downf = up.float(), down.float()   # the casts of the factors are not charged to the composition

                def composed():
                    return ops.quantize_weight(torch.addmm(ops.dequant(qw, torch.float32, 0, use_svd=False), upf, downf, alpha=S), wdt, qw.group_size)

                def fused():
                    return ops.merge_lowrank(qw, up, down, S, weights_dtype=wdt)
                ref, got = composed(), fused()
                diff = int((ref[0].contiguous().view(torch.uint8) != got[0].contiguous().view(torch.uint8)).sum())
                r = race({"kernel": fused, "composed": composed}, iters, rounds)
                spread, codes = spread_of(r["composed"]), stored_bytes(qw)
                line = dict(bench="merge_lowrank", weights=fmt, n=n, k=k, rank=rank, dtype="bf16", kernel_us=med(r["kernel"]),
                            kernel_min_us=round(min(r["kernel"]), 2), composed_us=med(r["composed"]), composed_min_us=round(min(r["composed"]), 2),
                            spread=spread, kernel_spread=spread_of(r["kernel"]), ratio=round(med(r["kernel"]) / med(r["composed"]), 3),
                            codes_bytes=codes, codes_bytes_per_s=round(codes / (med(r["kernel"]) * 1e-6)), code_bytes_differing=diff,
                            code_bytes_total=ref[0].numel() * ref[0].element_size(), device=torch.cuda.get_device_name(0))
                emit(out, line)
                if med(r["kernel"]) > med(r["composed"]) * (1 + spread):
                    lost.append(line)
                del ref, got
            del qw
            torch.cuda.empty_cache()
    return lost


def sdxl_model(layers):
    cfg = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    mods = torch.nn.ModuleList()
    for i, (_, _, k, n, _, count) in enumerate(layers):
        for j in range(count):
            mods.append(quantized(k, n, cfg, seed=1000 * i + j))
    sdnq_amd.accelerate(mods)
    return mods


def merge_once(layers, composition):
    mods = sdxl_model(layers)
    res = sdnq_amd.add_lora(mods, rank=16, seed=1)
    g = torch.Generator(device=DEV).manual_seed(2)
    with torch.no_grad():
        for p in res.parameters[1::2]:
            p.copy_(torch.randn(p.shape, device=DEV, dtype=p.dtype, generator=g) * 0.05)
    lora._MERGE_FORCE_COMPOSITION = composition
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        merged = sdnq_amd.merge_lora(mods)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        lora._MERGE_FORCE_COMPOSITION = False
    assert merged == len(mods) == int(res), (int(merged), len(mods), int(res))
    nbytes = sum(stored_bytes(linear._state(m).qw) for m in mods)
    del mods
    torch.cuda.empty_cache()
    return dt, int(merged), nbytes


def bench_sdxl(out):
    layers = shapes.sdxl_unet_linears()
    for composition in (False, True):
        merge_once(layers[-2:], composition)  # warm-up: first-call costs of both routes
    fused_s, count, nbytes = merge_once(layers, False)
    composed_s, _, _ = merge_once(layers, True)
    emit(out, dict(bench="merge_lora_sdxl_step", weights="int8_rowwise", rank=16, dtype="bf16", layers=count, codes_bytes=nbytes,
                   merge_lora_s=round(fused_s, 4), composition_s=round(composed_s, 4), ratio=round(fused_s / composed_s, 3),
                   per_layer_us=round(fused_s / count * 1e6, 1), runs=1, device=torch.cuda.get_device_name(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "merge_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("merge", "sdxl"))
    ap.add_argument("--weights", choices=sorted(FORMATS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("merge_bench.py measures on the GPU; none is visible")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        lost = bench_merge(f, a.iters, a.rounds, [a.weights] if a.weights else list(FORMATS)) if a.only != "sdxl" else []
        if a.only != "merge":
            bench_sdxl(f)
    if lost:
        sys.exit("ops.merge_lowrank is slower than dequant + addmm + quantize_weight beyond the spread at: "
                 + ", ".join(f"{ln['weights']} {ln['n']}x{ln['k']} rank {ln['rank']}" for ln in lost))


if __name__ == "__main__":
    main()
