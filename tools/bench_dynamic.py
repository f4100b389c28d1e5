#!/usr/bin/env python3
"""Dynamic quantization (use_dynamic_quantization=True) on the MI355X, one JSON line per measurement (results:
profiles/dynamic_quant_bench.md):

  loss    the fused loss kernel (ops.dequant_loss_sum: sdnq_hip_dequant_loss, one pass + a fixed-order sum) against torch's
          F.mse_loss(ref, ops.dequant(...)) on the same GPU, at FLUX Linear shapes, for 4-bit group-wise, 8-bit row-wise, SVD r=32 and
          Hadamard 256 weights; achieved bytes/s over the algorithmic bytes NK * (ref bytes + bits / 8) + 4 N G (x2 with zero points)
          + SVD factors, and the share of 8 TB/s.  Both losses are printed.
  search  one layer's whole dtype search, HIP (quantize + fused loss + one host sync per candidate) against the torch formulation
          on the same GPU (torch quantizer, torch dequantize, F.mse_loss), with a threshold that walks ~10 candidates; plus the
          cost of the host sync alone (a 0-dim device tensor read back).

Median microseconds over hipEvent-timed repeats after warm-up (search: wall-clock, synchronised).

    python tools/bench_dynamic.py [--repeats 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sdnq_amd import ops  # noqa: E402
from sdnq_amd import quantizer as Q  # noqa: E402
from sdnq_amd.common import dtype_dict  # noqa: E402
from sdnq_amd.quant_utils import dequantize_host  # noqa: E402

SHAPES = {"flux_qkv": (9216, 3072), "flux_mlp_up": (12288, 3072), "flux_mlp_down": (3072, 12288)}  # (N, K)
CONFIGS = {"uint4_g32": dict(weights_dtype="uint4", group_size=32), "int8_rowwise": dict(weights_dtype="int8", group_size=-1),
           "int4_svd32": dict(weights_dtype="int4", use_svd=True, svd_rank=32), "int4_had256": dict(weights_dtype="int4", use_hadamard=True)}


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


def wall(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    times.sort()
    return times[len(times) // 2]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def bench_loss(args, out, dev):
    for sname, (n, k) in SHAPES.items():
        torch.manual_seed(0)
        ref = (torch.randn(n, k, device=dev) * 0.02).to(torch.bfloat16)
        for cname, cfg in CONFIGS.items():
            dq, t = Q.sdnq_quantize_layer_weight(ref, "Linear", **cfg)
            qw = dq.quant_weight(t["weight"], t["scale"], t["zero_point"], t["svd_up"], t["svd_down"])
            had = dq.hadamard_group_size if dq.use_hadamard else 0
            fused = timed(lambda: ops.dequant_loss_sum(qw, ref, had), args.warmup, args.repeats)
            eager = timed(lambda: torch.nn.functional.mse_loss(ref.float(), ops.dequant(qw, torch.float32, had)), args.warmup, args.repeats)
            bits = dtype_dict[dq.weights_dtype]["num_bits"]
            groups = k // dq.group_size if dq.group_size > 0 else 1
            nbytes = n * k * (ref.element_size() + bits / 8) + 4 * n * groups * (2 if t["zero_point"] is not None else 1)
            if t["svd_up"] is not None:
                nbytes += (t["svd_up"].numel() + t["svd_down"].numel()) * t["svd_up"].element_size()
            loss_fused = float(ops.dequant_loss_sum(qw, ref, had)) / ref.numel()
            loss_eager = float(torch.nn.functional.mse_loss(ref.float(), ops.dequant(qw, torch.float32, had)))
            emit(dict(bench="loss", shape=sname, n=n, k=k, config=cname, weights_dtype=dq.weights_dtype, group_size=dq.group_size,
                      fused_us=round(fused, 2), torch_us=round(eager, 2), speedup=round(eager / fused, 2), alg_bytes=int(nbytes),
                      fused_TBps=round(nbytes / fused / 1e6, 3), share_of_8TBps=round(nbytes / fused / 1e6 / 8.0, 3),
                      mse_fused=loss_fused, mse_torch=loss_eager), out)


def torch_search(w, start, threshold):
    """The reference's formulation on the same GPU: torch quantizer, torch dequantize, F.mse_loss, one sync per candidate."""
    original = w.float()
    std = original.std().square_().clamp_(min=1e-8)
    order = Q.weights_dtype_order
    hip = Q.USE_HIP_QUANTIZER
    Q.USE_HIP_QUANTIZER = False
    try:
        for i, cur in enumerate(order[order.index(start):]):
            dq, t = Q.sdnq_quantize_layer_weight(original, "Linear", weights_dtype=cur)
            deq = dequantize_host(dq, t["weight"], t["scale"], t["zero_point"], None, None)
            if bool(torch.nn.functional.mse_loss(original, deq).div_(std) <= threshold):
                return cur, i + 1
    finally:
        Q.USE_HIP_QUANTIZER = hip
    return "float", i + 1


def bench_search(args, out, dev):
    n, k = SHAPES["flux_mlp_up"]
    torch.manual_seed(1)
    w = (torch.randn(n, k, device=dev) * 0.02).to(torch.bfloat16)
    start, threshold = "int2", 2e-4  # walks int2 .. ~int6 (about ten candidates)
    trace = []
    real = Q._candidate_mse

    def spy(dq, data, original, ref):
        out_ = real(dq, data, original, ref)
        trace.append(dq.weights_dtype)
        return out_

    Q._candidate_mse = spy
    try:
        res = Q.sdnq_quantize_layer_weight_dynamic(w, "Linear", weights_dtype=start, dynamic_loss_threshold=threshold)
    finally:
        Q._candidate_mse = real
    chosen, cands = res[0].weights_dtype, len(trace)
    hip_us = wall(lambda: Q.sdnq_quantize_layer_weight_dynamic(w, "Linear", weights_dtype=start, dynamic_loss_threshold=threshold),
                  1, max(3, args.repeats // 4))
    t_chosen, t_cands = torch_search(w, start, threshold)
    torch_us = wall(lambda: torch_search(w, start, threshold), 1, max(3, args.repeats // 4))
    x = torch.zeros((), device=dev, dtype=torch.float32)
    sync_us = wall(lambda: bool(x <= 1.0), args.warmup, args.repeats * 10)
    emit(dict(bench="search", n=n, k=k, start=start, threshold=threshold, chosen=chosen, candidates=cands, torch_chosen=t_chosen,
              torch_candidates=t_cands, hip_us=round(hip_us, 1), torch_us=round(torch_us, 1), speedup=round(torch_us / hip_us, 2),
              hip_us_per_candidate=round(hip_us / cands, 1), torch_us_per_candidate=round(torch_us / t_cands, 1),
              host_sync_us=round(sync_us, 1)), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    emit(dict(bench="device", name=torch.cuda.get_device_name(0)), out)
    bench_loss(args, out, dev)
    bench_search(args, out, dev)


if __name__ == "__main__":
    main()
