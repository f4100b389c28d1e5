#!/usr/bin/env python3
"""Golden vectors for the quantized attention backward (sdnq_amd.attention.sdnq_hip_atten_with_backward), made by RUNNING the reference's
own Triton kernels (`sdnq_attn_bwd_dq_kernel`, `sdnq_attn_bwd_dkv_kernel`, kernels/triton_atten_backward.py:139-483) and its host code
(`sdnq_triton_atten(return_backward=True)`, `sdnq_triton_atten_bwd`, :728-841) on the CPU through Triton's interpreter, with the harness
of make_golden_attention.py (one fixed 32 x 32 block configuration in place of the autotuner, wrap_triton as the identity, fp32 scalar
handles for Python floats).  Files are prefixed ``abwd_`` (``attn_*`` are the forward's fixtures).

What this harness adds for the backward:
  * padded head dims (40, 80): the reference's get_attn_backward_inputs multiplies the padded saved `out` with the unpadded grad_output
    (a shape mismatch in the reference); the harness zero-pads grad_output to the padded head dim, which is what the kernels read;
  * the bf16_* cases use the forward generator's trick: quantize_attn runs on the real bfloat16 tensors, the kernels run with V, dO, out
    and lse as float32 (meta "grads_are": P, out, lse and the gradients are NOT rounded to bfloat16);
  * query counts are multiples of 8 where a case has several heads: the interpreter's tensor descriptors want 16-byte aligned bases for
    the per-head float16 lse rows;
  * `exact_dq` / `exact_dk` / `exact_dv`: fp32 autograd through torch's SDPA on the same (rounded) inputs -- the baseline both
    implementations are measured against.
Fixtures are DATA only.  Run:  python tests/golden/make_golden_attention_backward.py [case ...]
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_attention as fwd  # noqa: E402  (sets up the interpreter harness and imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdnq.kernels import triton_atten_backward as tb  # noqa: E402  (the reference)

ta = fwd.ta
tb.wrap_triton = lambda k: k
tb.sdnq_attn_bwd_dq_kernel = fwd.FixedConfig(tb.sdnq_attn_bwd_dq_kernel.fn)
tb.sdnq_attn_bwd_dkv_kernel = fwd.FixedConfig(tb.sdnq_attn_bwd_dkv_kernel.fn)

CASES = [
    dict(name="f16_d64_tail", z=1, qh=2, kh=2, qn=40, kn=52, d=64, kw={}),
    dict(name="f16_d64_causal_tail", z=1, qh=1, kh=1, qn=44, kn=44, d=64, kw=dict(is_causal=True)),
    dict(name="f16_d128_gqa", z=1, qh=4, kh=2, qn=40, kn=68, d=128, kw={}),
    dict(name="f16_d64_nosmooth_scale", z=1, qh=2, kh=1, qn=40, kn=100, d=64, kw=dict(smooth_k=False, scale=0.2)),
    dict(name="f16_d64_long", z=1, qh=1, kh=1, qn=132, kn=260, d=64, kw={}),
    dict(name="f16_d64_boolmask", z=2, qh=2, kh=2, qn=40, kn=80, d=64, kw={}, mask=dict(kind="bool", shape=(2, 1, 40, 80), dead_rows=(3, 17))),
    dict(name="f16_d64_floatmask_2d_causal", z=1, qh=2, kh=1, qn=48, kn=48, d=64, kw=dict(is_causal=True), mask=dict(kind="f16", shape=(48, 48))),
    dict(name="f16_d40_padded", z=1, qh=2, kh=2, qn=40, kn=56, d=40, kw={}),
    dict(name="f16_d80_padded_causal", z=1, qh=2, kh=1, qn=40, kn=40, d=80, kw=dict(is_causal=True)),
    dict(name="f16_d64_hadamard", z=1, qh=2, kh=2, qn=48, kn=72, d=64, kw=dict(use_hadamard=True)),
    dict(name="f16_d128_hadamard_g32", z=1, qh=2, kh=1, qn=40, kn=40, d=128, kw=dict(use_hadamard=True, hadamard_group_size=32, is_causal=True)),
    dict(name="bf16_d64_tail", dtype="bf16", z=1, qh=2, kh=2, qn=40, kn=52, d=64, kw={}),
    dict(name="bf16_d128_gqa_causal", dtype="bf16", z=1, qh=4, kh=2, qn=44, kn=44, d=128, kw=dict(is_causal=True)),
]


def make_inputs(case):
    g = torch.Generator().manual_seed(sum(map(ord, "abwd_" + case["name"])))
    z, qh, kh, qn, kn, d = (case[k] for k in ("z", "qh", "kh", "qn", "kn", "d"))
    q = torch.randn(z, qh, qn, d, generator=g)
    k = torch.randn(z, kh, kn, d, generator=g) + 3.0 * torch.randn(1, kh, 1, d, generator=g)
    v = torch.randn(z, kh, kn, d, generator=g)
    do = torch.randn(z, qh, qn, d, generator=g)
    q[..., 5] *= 6.0
    tdt = torch.bfloat16 if case.get("dtype", "f16") == "bf16" else torch.float16
    q, k, v, do = q.to(tdt), k.to(tdt), v.to(tdt), do.to(tdt)
    mask = None
    if "mask" in case:
        ms = case["mask"]
        if ms["kind"] == "bool":
            mask = torch.rand(ms["shape"], generator=g) > 0.35
            for r in ms.get("dead_rows", ()):
                mask[..., r, :] = False
            mask[..., 32:64] &= torch.rand(ms["shape"][:-1] + (1,), generator=g) > 0.5
        else:
            mask = torch.randn(ms["shape"], generator=g) * 2.0
            mask[torch.rand(ms["shape"], generator=g) < 0.2] = float("-inf")
            mask[..., 0] = 0.5
            mask = mask.to(tdt if ms["kind"] == "f16" else torch.float32)
    return q, k, v, do, mask


def exact_grads(q, k, v, do, mask, case):
    """fp32 autograd through torch's SDPA on the rounded inputs (dead rows of a bool mask: zero, as the quantized kernels give)."""
    rep = case["qh"] // case["kh"]
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    m, causal = mask, case["kw"].get("is_causal", False)
    if m is not None:
        if m.dtype != torch.bool:  # the reference adds a float mask in the log2(e)-scaled domain: exp2(s log2(e) + m) = exp(s + m ln 2)
            m = m.float() * math.log(2.0)
        if causal:
            tri = torch.ones(case["qn"], case["kn"], dtype=torch.bool).triu(1)
            m = m.masked_fill(tri, False) if m.dtype == torch.bool else m.masked_fill(tri, float("-inf"))
            causal = False
    out = torch.nn.functional.scaled_dot_product_attention(qf, kf.repeat_interleave(rep, 1), vf.repeat_interleave(rep, 1), attn_mask=m,
                                                           is_causal=causal, scale=case["kw"].get("scale"))
    out = torch.nan_to_num(out, nan=0.0)
    out.backward(do.float())
    return [torch.nan_to_num(t.grad, nan=0.0) for t in (qf, kf, vf)]


def run(case):
    q, k, v, do, mask = make_inputs(case)
    kw = dict(case["kw"])
    bf16 = case.get("dtype", "f16") == "bf16"
    captured = {}
    real_quantize = ta.quantize_attn
    if bf16:
        def on_bf16(q_, k_, v_, smooth_k=True, hadamard=None, **kw_):
            r = list(real_quantize(q_.to(torch.bfloat16), k_.to(torch.bfloat16), v_.to(torch.bfloat16), smooth_k=smooth_k,
                                   hadamard=None if hadamard is None else hadamard.to(torch.bfloat16), **kw_))
            r[4] = r[4].float()
            captured["r"] = tuple(r)
            return tuple(r)
        ta.quantize_attn = on_bf16
    try:
        src = (q.float(), k.float(), v.float()) if bf16 else (q, k, v)
        (out, lse, q_q, k_q, v_q, q_s, k_s, v_s, mask_p, _scale, use_h, hg) = ta.sdnq_triton_atten(*src, attn_mask=mask, return_backward=True, **kw)
    finally:
        ta.quantize_attn = real_quantize
    d = case["d"]
    dpad = out.shape[-1]
    grad = do.float() if bf16 else do
    if dpad != d:
        grad = torch.nn.functional.pad(grad, (0, dpad - d))
    dq, dk, dv = tb.sdnq_triton_atten_bwd(grad, out, lse, q_q, k_q, v_q, q_s, k_s, v_s, d, d, d, attn_mask=mask_p,
                                          sm_scale=kw.get("scale"), is_causal=kw.get("is_causal", False), use_hadamard=use_h,
                                          hadamard_group_size=hg)
    edq, edk, edv = exact_grads(q, k, v, do, mask, case)
    arrays, meta = {}, {"name": case["name"], "dtype": case.get("dtype", "f16"), "shape": {k_: case[k_] for k_ in ("z", "qh", "kh", "qn", "kn", "d")},
                        "kwargs": case["kw"], "block_m": fwd.BLOCK_M, "block_n": fwd.BLOCK_N, "hadamard_group": int(hg) if use_h else 0,
                        "tensors": {},
                        **({"grads_are": "float32: the reference kernels on the bfloat16 path's quantized operands with V, dO, out and lse as "
                                         "float32 (P, out, lse and the gradients unrounded)"} if bf16 else {})}
    tensors = [("q", q), ("k", k), ("v", v), ("do", do), ("out", out[..., :d]), ("lse", lse), ("q_q", q_q), ("q_scale", q_s),
               ("k_q", k_q[..., :dpad]), ("k_scale", k_s), ("dq", dq), ("dk", dk), ("dv", dv),
               ("exact_dq", edq), ("exact_dk", edk), ("exact_dv", edv)] + ([("mask", mask)] if mask is not None else [])
    for key, t in tensors:
        arrays[key], tag = fwd.bits(t)
        meta["tensors"][key] = {"dtype": tag, "shape": list(t.shape)}
    np.savez_compressed(os.path.join(HERE, f"abwd_{case['name']}.npz"), **arrays)
    with open(os.path.join(HERE, f"abwd_{case['name']}.json"), "w") as f:
        json.dump(meta, f, indent=1)
    rel = [float((a.float() - b).norm() / b.norm()) for a, b in ((dq, edq), (dk, edk), (dv, edv))]
    print("wrote abwd", case["name"], "rel L2 vs fp32 SDPA (dq, dk, dv):", ", ".join(f"{r:.3g}" for r in rel))


if __name__ == "__main__":
    only = sys.argv[1:] or None
    for c in CASES:
        if only is None or c["name"] in only:
            run(c)
