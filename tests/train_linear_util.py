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


# ---- the column quantizer at training size (tests/test_colquant_exact_gpu.py) -----------------------------------------------------
MAX_SLABS = 32
TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def cq_plan(r, c):
    """(ctiles, nslab, slab_rows): cq_plan of csrc/colquant.hip restated -- how the statistics pass cuts R rows into slabs.  It only
    documents and asserts which regime a test shape reaches; test_train_linear_host.py ties it to the library's workspace size."""
    ctiles = -(-c // COLUMN_TILE)
    want = min(-(-512 // ctiles), MAX_SLABS)
    nslab = min(want, (r + 31) // 32)
    slab_rows = (-(-r // nslab) + STAT_SLAB_ROWS - 1) // STAT_SLAB_ROWS * STAT_SLAB_ROWS
    return ctiles, -(-r // slab_rows), slab_rows


def row_tiles(r):
    """Row tiles of colquant_t_kernel at the ld_t ops.colquant_t allocates."""
    return -(-((r + 15) // 16 * 16) // ROW_TILE)


# (R, C) -> the regime it reaches: slabs and 128-row passes per slab of colstat_kernel, rows in the last slab, row tiles of
# colquant_t_kernel, column tiles, and the slab count the plan asks for before the rows cap it (want < 32: many column tiles)
CENSUS_SHAPES = {
    (3969, 8): dict(nslab=32, passes=1, last_slab=1, row_tiles=16, ctiles=1, want=32),        # one column lane of eight works
    (4097, 72): dict(nslab=17, passes=2, last_slab=1, row_tiles=17, ctiles=2, want=32),       # last row tile holds 1 row; partial column tile
    (8200, 24): dict(nslab=22, passes=3, last_slab=136, row_tiles=33, ctiles=1, want=32),
    (4100, 2056): dict(nslab=11, passes=3, last_slab=260, row_tiles=17, ctiles=33, want=16),
    (260, 32712): dict(nslab=1, passes=3, last_slab=260, row_tiles=2, ctiles=512, want=1),
}
EDGE_SHAPES = {
    (1280, 16): dict(nslab=10, passes=1, last_slab=128, row_tiles=5, ctiles=1, want=32),      # ties and near-ties per column
    (1536, 208): dict(nslab=12, passes=1, last_slab=128, row_tiles=6, ctiles=4, want=32),     # the exponent range per column
}


def regime(r, c):
    ctiles, nslab, slab_rows = cq_plan(r, c)
    return dict(nslab=nslab, passes=slab_rows // STAT_SLAB_ROWS, last_slab=r - (nslab - 1) * slab_rows, row_tiles=row_tiles(r),
                ctiles=ctiles, want=min(-(-512 // ctiles), MAX_SLABS))


def census_pin_rows(r, c):
    """[C] the row of each column's +-127, cycling over row 0, row R - 1 (alone in the last slab at R = 3969 and 4097) and, where a slab
    has a second 128-row pass, the first rows of the second or a later pass of some slab (slab_start + 128 p + 0..3)."""
    _, nslab, slab_rows = cq_plan(r, c)
    later = [s * slab_rows + STAT_SLAB_ROWS * p for s in range(nslab) for p in range(1, slab_rows // STAT_SLAB_ROWS)
             if s * slab_rows + STAT_SLAB_ROWS * p + 3 < r]
    rows = torch.zeros(c, dtype=torch.int64)
    for col in range(c):
        kind = col % (3 if later else 2)
        rows[col] = (0, r - 1, later[col // 3 * 7 % len(later)] + col % 4 if later else 0)[kind]
    return rows


def exact_matrix(r, c, gen, exp, pin_rows):
    """(x float32 [R][C], q int8 [R][C], e int64 [C]) with x = q * 2^e[c]: 1 <= |q| <= 8 with a random sign -- no zero, so a dropped or
    doubled row changes every column sum -- except one +-127 per column at pin_rows[c].  e[c] is `exp` (an int, or [C]) or, for None, drawn
    from -3..3.  127 * 2^e / 127 = 2^e in IEEE arithmetic, so the column quantizer's codes are q and its scales 2^e, and the column sums are
    integers below 2^24 times 2^e: exact in float32 in every order.  Every x is a bf16 and a float16 value (7 bits, |x| <= 1016)."""
    q = torch.randint(1, 9, (r, c), generator=gen) * (torch.randint(0, 2, (r, c), generator=gen) * 2 - 1)
    q[pin_rows, torch.arange(c)] = 127 * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1)
    e = torch.randint(-3, 4, (c,), generator=gen) if exp is None else torch.as_tensor(exp, dtype=torch.int64).expand(c)
    return q.float() * torch.exp2(e.float()), q.to(torch.int8), e


def exact_operand(r, c, gen, exp):
    """(x float32 [R][C], q int8) with x = q * 2^exp: |q| <= 8 apart from a +127 in every row (at column i mod C) and a -127 in every
    column (at row (j + 1) mod R), so that the row scales AND the column scales are exactly 2^exp and the codes are q either way."""
    q = torch.randint(-8, 9, (r, c), generator=gen)
    rows, cols = torch.arange(r), torch.arange(c)
    q[rows, rows % c] = 127
    assert (((cols + 1) % r) % c != cols).all()  # a -127 never lands on a +127
    q[(cols + 1) % r, cols] = -127
    assert (q.abs().amax(0) == 127).all() and (q.abs().amax(1) == 127).all()
    return q.float() * 2.0 ** exp, q.to(torch.int8)


def _oracle():
    from oracle import oracle
    return oracle


def oracle_colquant_t(x2d):
    """(codes int8 [C][ld_t], scale float32 [C][1]) of the column quantizer from the C oracle's ROW quantizer on the transposed matrix:
    an implementation that shares nothing with `quantize` above."""
    r, c = x2d.shape
    q, s, _ = _oracle().rowquant(x2d.float().t().contiguous().numpy(), "int8")
    q_t = torch.zeros(c, (r + 15) // 16 * 16, dtype=torch.int8)
    q_t[:, :r] = torch.from_numpy(q)
    return q_t, torch.from_numpy(s).reshape(c, 1)


def oracle_chain(x, w, bias, dy, dtype):
    """(y, grad_input, grad_weight) in `dtype` from the C oracle alone: oracle.rowquant on each operand or its transpose, then
    oracle.scaled_mm("int8", ...).  x [M][K], w [N][K], dy [M][N]."""
    O, tag = _oracle(), TAG[dtype]

    def rowq(t):
        return O.rowquant(t.float().contiguous().numpy(), "int8")[:2]

    def mm(a, b, sa, sb, b_=None):
        return torch.from_numpy(O.scaled_mm("int8", a, b, sa, sb, b_, tag)).to(dtype)  # values of `dtype` already: the cast is exact
    (xq, xs), (wq, ws), (gq, gs) = rowq(x), rowq(w), rowq(dy)
    (wq_t, wsc), (gq_t, gsc), (xq_t, xsc) = rowq(w.t()), rowq(dy.t()), rowq(x.t())
    y = mm(xq, wq, xs, ws, None if bias is None else bias.float().numpy())
    return y, mm(gq, wq_t, gs, wsc), mm(gq_t, xq_t, gsc, xsc)  # (reducing over M instead of M': the pad columns are zero codes)


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
