"""A CPU restatement, in torch, of the int8 training Linear (sdnq_amd.training; the reference's int8_matmul_dynamic_with_backward,
training/layers/linear/linear_int8/linear_int8_dynamic.py):

  quantize(x, dim):   scale = amax(|x|, dim) / 127 in float32;  codes = clamp(round_half_even(x / scale), -128, 127)      (quantize_int_mm)
  colquant_t(x2d):    quantize(x2d, 0) with the codes transposed to [C][ld_t], ld_t = R rounded up to 16, pad columns zero; colsum in float32
  scaled_mm:          out[m][n] = cast(fma(f32(sum_k a[m][k] b[n][k]) * sa[m], sb[n], bias[n]))                 (sdnq_hip_scaled_mm's epilogue)
  y           = scaled_mm(quantize(x, -1), quantize(W, -1), bias)
  grad_input  = scaled_mm(quantize(dY, -1), colquant_t(W))
  grad_weight = scaled_mm(colquant_t(dY), colquant_t(x))          reducing over ld_t; the pad columns add nothing
  grad_bias   = cast(colsum(dY))
and the loading of the fixtures tests/golden/train_int8_* (tests/golden/make_golden_training.py).
"""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# the geometry of csrc/colquant.hip that the fixture shapes are chosen against
COLUMN_TILE, STAT_SLAB_ROWS, ROW_TILE = 64, 128, 256


def train_names():
    return sorted(f[len("train_int8_"):-5] for f in os.listdir(GOLD) if f.startswith("train_int8_") and f.endswith(".json"))


def load(name):
    """(meta, {key: tensor}) of one fixture; 16-bit floats come back in their dtype."""
    meta = json.load(open(os.path.join(GOLD, f"train_int8_{name}.json")))
    z = np.load(os.path.join(GOLD, f"train_int8_{name}.npz"))
    out = {}
    for key, info in meta["tensors"].items():
        t = torch.from_numpy(np.ascontiguousarray(z[key]))
        if info["dtype"] in ("bf16", "f16"):
            t = t.view(TORCH_DT[info["dtype"]])
        out[key] = t.reshape(info["shape"])
    return meta, out


def quantize(x, dim):
    """quantize_int_mm(x.float(), dim) -> (codes int8, scale float32 with `dim` kept)."""
    x = x.float()
    scale = x.abs().amax(dim=dim, keepdim=True) / 127
    q = torch.where(scale == 0, torch.zeros_like(x), torch.round(x / scale))  # a zero column: scale 0, codes 0 (the kernels' convention)
    return q.clamp(-128, 127).to(torch.int8), scale


def colquant_t(x2d, want_colsum=False):
    """(codes [C, ld_t] int8, scale [C, 1] float32, colsum [C] float32 | None) as ops.colquant_t returns them."""
    r, c = x2d.shape
    q, scale = quantize(x2d, 0)
    ld_t = (r + 15) // 16 * 16
    q_t = torch.zeros(c, ld_t, dtype=torch.int8)
    q_t[:, :r] = q.t()
    colsum = x2d.float().sum(0, dtype=torch.float32) if want_colsum else None
    return q_t, scale.reshape(c, 1), colsum


def scaled_mm(a, b_phys, sa, sb, bias, dtype):
    acc = (a.double() @ b_phys.double().t()).float()  # integers below 2^24 * 2^7: exact in float64, and in float32 for these K
    t = (acc * sa.reshape(-1, 1).float()).double() * sb.reshape(1, -1).double()
    if bias is not None:
        t = t + bias.double().reshape(1, -1)
    return t.float().to(dtype)


def forward(x, w, bias):
    x2d = x.reshape(-1, x.shape[-1])
    xq, xs = quantize(x2d, -1)
    wq, ws = quantize(w, -1)
    return scaled_mm(xq, wq, xs, ws, bias, x.dtype).reshape(*x.shape[:-1], w.shape[0])


def backward(x, w, dy, need=(True, True, True)):
    x2d, g2d = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
    gi = gw = gb = None
    if need[0]:
        gq, gs = quantize(g2d, -1)
        wq_t, wsc, _ = colquant_t(w)
        gi = scaled_mm(gq, wq_t, gs, wsc, None, dy.dtype).reshape(x.shape)
    if need[1]:
        gq_t, gs_t, _ = colquant_t(g2d)
        xq_t, xsc, _ = colquant_t(x2d)
        gw = scaled_mm(gq_t, xq_t, gs_t, xsc, None, dy.dtype)
    if need[2]:
        gb = colquant_t(g2d, want_colsum=True)[2].to(dy.dtype)
    return gi, gw, gb


# ---- the bounds of the issue's checks ---------------------------------------------------------------------------------------------
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -23}
REL_L2 = {torch.bfloat16: 2e-3, torch.float16: 2e-3, torch.float32: 1e-5}
HALF_SPACING = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}  # of a value in [1, 2)


def w8a8_errors(got, ref):
    """(max |err| / max |ref|, rel-L2): the project's standing w8a8 measure (header of tests/test_gpu_parity.py)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = float(ref.abs().max()) or 1.0
    return float((got - ref).abs().max()) / scale, float((got - ref).norm() / (ref.norm() or 1.0))


def assert_w8a8_close(got, ref, what):
    """|err| <= 2 ulp(out dtype) of the output's magnitude scale, rel-L2 <= 2e-3 (bf16, f16) / 1e-5 (f32)."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    err, l2 = w8a8_errors(got, ref)
    print(what, "max err / scale", err, "rel l2", l2)
    assert err <= 2 * ULP[ref.dtype], (what, "max err / scale", err, 2 * ULP[ref.dtype])
    assert l2 <= REL_L2[ref.dtype], (what, "rel l2", l2)


def colsum_bound(x2d):
    """Per column: 0.5 ulp_f32(|s|) + R * 2^-24 * sum_r |x[r][c]| around the float64 column sum s -- float32 accumulation of R terms."""
    xd = x2d.double().cpu()
    s = xd.sum(0)
    ulp = torch.exp2(torch.floor(torch.log2(s.abs().clamp(min=2.0 ** -126))) - 23)
    return s, 0.5 * ulp + x2d.shape[0] * 2.0 ** -24 * xd.abs().sum(0)


def grad_bias_bound(dy2d, dtype):
    """(float64 column sums, bound): colsum_bound plus one rounding of a value of that size to `dtype`."""
    s, bound = colsum_bound(dy2d)
    return s, bound + torch.exp2(torch.floor(torch.log2((s.abs() + bound).clamp(min=2.0 ** -14)))) * HALF_SPACING[dtype]
