#!/usr/bin/env python3
"""The fused AdamW step (sdnq_amd.optim, csrc/optim.hip) on parameter tensors of the SDXL and FLUX projection sizes, bf16 and float32,
with dense and with uint8 state, deterministic rounding everywhere:

  hip          one ops.adamw_step / ops.adamw_step_q8 call
  hip_sr       the same with stochastic rounding of everything 16-bit / uint8 (the optimizer's defaults): the cost of the random numbers
  torch_ops    (a) the same arithmetic written in torch ops on the device: nan_to_num, clamp, lerp_, div, rsqrt, mul, add_, copy_ -- and
               for uint8 state addcmul, aminmax, sub, div, round, clamp, to(uint8) -- about 20 / 35 launches
  torch_fused  (b) torch.optim.AdamW(fused=True).step() on the same parameter (dense state only; its own arithmetic: eps, no clamps)

Timing: eager calls on the default stream, `--iters` calls between two device events, `--rounds` rounds with the contenders in
alternation after a warm-up round; median and min per call.  bytes_per_el is what the algorithm has to move by design -- dense: the
parameter and both moments read and written, the gradient read (7 x element size); uint8 state: parameter read and written, gradient
read, two codes read and written, scale and zero point of both buffers read and written per 32 elements (3 x element size + 5) -- and
gb_per_s is that over the measured time.  One JSON line per (shape, dtype, state form), written to --out.
Exit status 1 if `hip` is slower than `torch_ops` anywhere.
Usage: python tools/optim_bench.py [--out profiles/optim_adamw_bench.jsonl] [--iters 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdnq_amd import ops  # noqa: E402
from sdnq_amd.optim import QuantizedBuffer  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(640, 640), (5120, 640), (3072, 12288), (16384, 5120)]
LR, BETAS, WD, CLIP, STEP = 1e-4, (0.9, 0.999), 0.01, 1.0, 3


def torch_dense(p, g, m, v):
    b1, b2 = BETAS
    g32 = torch.nan_to_num(g).float().clamp_(-CLIP, CLIP)
    p32 = torch.nan_to_num(p).float()
    m32 = m.float().lerp_(g32, 1 - b1) if m.dtype != torch.float32 else m.lerp_(g32, 1 - b1)
    v32 = v.float().lerp_(g32.square(), 1 - b2) if v.dtype != torch.float32 else v.lerp_(g32.square(), 1 - b2)
    if m.dtype != torch.float32:
        m.copy_(m32)
        v.copy_(v32)
    u = (m32 / (1 - b1 ** STEP)).mul_((v32 / (1 - b2 ** STEP)).rsqrt_()).nan_to_num_().clamp_(-CLIP, CLIP)
    p32.mul_(1 - LR * WD).add_(u, alpha=-LR)
    p.copy_(p32)


def _requant(buf: QuantizedBuffer, x32):
    xg = x32.view(buf.weight.shape)
    lo, hi = torch.aminmax(xg, dim=-1, keepdim=True)
    scale = hi.sub_(lo).div_(255.0)
    buf.weight.copy_(torch.sub(xg, lo).div_(scale).round_().nan_to_num_().clamp_(0, 255))
    buf.scale.copy_(scale)
    buf.zero_point.copy_(lo)


def torch_q8(p, g, m: QuantizedBuffer, v: QuantizedBuffer):
    b1, b2 = BETAS
    g32 = torch.nan_to_num(g).float().clamp_(-CLIP, CLIP)
    p32 = torch.nan_to_num(p).float()
    m32 = m.dequantize().lerp_(g32, 1 - b1)
    _requant(m, m32)
    v32 = v.dequantize().lerp_(g32.square(), 1 - b2)
    _requant(v, v32)
    u = (m32 / (1 - b1 ** STEP)).mul_((v32 / (1 - b2 ** STEP)).rsqrt_()).nan_to_num_().clamp_(-CLIP, CLIP)
    p32.mul_(1 - LR * WD).add_(u, alpha=-LR)
    p.copy_(p32)


def race(fns: dict, iters, rounds):
    """{name: (median us, min us)} per call; the contenders alternate, the first round is a warm-up."""
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) * 1000.0 / iters)
    return {k: (statistics.median(t), min(t)) for k, t in times.items()}


def bench(shape, dtype, quantized, iters, rounds):
    g = torch.Generator(device=DEV).manual_seed(1)
    n = shape[0] * shape[1]
    p0 = (torch.randn(shape, device=DEV, generator=g) * 0.5).to(dtype)
    grad = (torch.randn(shape, device=DEV, generator=g) * 0.3).to(dtype)
    kw = dict(step=STEP, lr=LR, betas=BETAS, weight_decay=WD, clip=CLIP)

    def state():
        m0, v0 = torch.randn(shape, device=DEV, generator=g) * 0.1, torch.rand(shape, device=DEV, generator=g) * 0.05
        if not quantized:
            return m0.to(dtype), v0.to(dtype)
        out = []
        for x in (m0, v0):  # a realistic quantized state: the torch composition's quantizer on random moments
            buf = QuantizedBuffer.zeros(shape, DEV)
            _requant(buf, x)
            out.append(buf)
        return out

    # the fused step against the torch composition on the same inputs, before anything is timed
    pa, pb, (ma, va), (mb, vb) = p0.clone(), p0.clone(), state(), state()
    if quantized:
        for dst, src in ((mb, ma), (vb, va)):
            for x, y in zip(dst.parts(), src.parts()):
                x.copy_(y)
        ops.adamw_step_q8(pa, grad, ma.parts(), va.parts(), **kw)
        torch_q8(pb, grad, mb, vb)
        moved = (ma.weight != mb.weight).float().mean().item()
        assert moved < 1e-2, f"codes differ from the torch composition in a share of {moved}"
    else:
        mb.copy_(ma)
        vb.copy_(va)
        ops.adamw_step(pa, grad, ma, va, **kw)
        torch_dense(pb, grad, mb, vb)
        for x, y in ((ma, mb), (va, vb)):
            assert (x.float() - y.float()).abs().max().item() <= 2.0 ** -7 * y.float().abs().max().item()
    assert (pa.float() - pb.float()).abs().max().item() <= 2.0 ** -7 * pb.float().abs().max().item(), "parameter differs from the torch composition"

    p, (m, v) = p0.clone(), state()
    fns = {}
    if quantized:
        fns["hip"] = lambda: ops.adamw_step_q8(p, grad, m.parts(), v.parts(), **kw)
        fns["hip_sr"] = lambda: ops.adamw_step_q8(p, grad, m.parts(), v.parts(), sr_param=True, sr_state=True, seed=1, offset=4, **kw)
        fns["torch_ops"] = lambda: torch_q8(p, grad, m, v)
    else:
        fns["hip"] = lambda: ops.adamw_step(p, grad, m, v, **kw)
        if dtype != torch.float32:
            fns["hip_sr"] = lambda: ops.adamw_step(p, grad, m, v, sr_param=True, sr_state=True, seed=1, offset=4, **kw)
        fns["torch_ops"] = lambda: torch_dense(p, grad, m, v)
        tp = torch.nn.Parameter(p0.clone())
        tp.grad = grad
        topt = torch.optim.AdamW([tp], lr=LR, betas=BETAS, weight_decay=WD, fused=True)
        fns["torch_fused"] = topt.step
    res = race(fns, iters, rounds)
    eb = p0.element_size()
    bytes_per_el = 3 * eb + 5 if quantized else 7 * eb
    line = dict(bench="adamw_step", shape=list(shape), dtype=str(dtype).replace("torch.", ""), state="uint8" if quantized else "dense",
                bytes_per_el=bytes_per_el, iters=iters, rounds=rounds)
    for k, (med, lo) in res.items():
        line[k + "_us"], line[k + "_min_us"] = round(med, 2), round(lo, 2)
    line["hip_gb_per_s"] = round(bytes_per_el * n / res["hip"][0] / 1e3, 1)
    line["torch_ops_over_hip"] = round(res["torch_ops"][0] / res["hip"][0], 2)
    if "torch_fused" in res:
        line["torch_fused_over_hip"] = round(res["torch_fused"][0] / res["hip"][0], 2)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_adamw_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    lost = []
    with open(a.out, "w") as f:
        for shape in SHAPES:
            for dtype in (torch.bfloat16, torch.float32):
                for quantized in (False, True):
                    line = bench(shape, dtype, quantized, a.iters, a.rounds)
                    print(json.dumps(line), flush=True)
                    f.write(json.dumps(line) + "\n")
                    f.flush()
                    if line["hip_us"] > line["torch_ops_us"]:
                        lost.append(line)
                    torch.cuda.empty_cache()
    if lost:
        sys.exit("the fused step is slower than the torch composition at: " + ", ".join(f"{ln['shape']} {ln['dtype']} {ln['state']}" for ln in lost))


if __name__ == "__main__":
    main()
