"""ops.norm_rowquant (csrc/normquant.hip) against the float64 restatement of its formula, against the row quantizer on its own y,
and against itself on another grid.

The bound of the first check, per element, with u = 2^-24 and the kernel's float32 chain (include/sdnq_hip.h):

    |y - ref| <= ulp_T(|ref| + E) / 2 + E,        E = u * (c * mag + (d + 1) * shifted)

* d = ceil(K / 512) + 9 bounds the additions any term of a reduction passes through: a lane's accumulator over the passes, the tree
  over a lane's 8 accumulators (3), the butterfly over 64 lanes (6).  A sum of K terms in that order is off by at most d u sum|t|.
* mean: d additions and a division, an ABSOLUTE error of (d + 1) u mean|x|.  It shifts every deviation of the row alike, so to first
  order it drops out of the variance (the deviations sum to zero); in y it stays as `shifted` = mean|x| r |weight| |1 + scale|.
* every other error is relative to the summands of z, `mag` = |n weight (1 + scale)| + |bias (1 + scale)| + |shift| >= |ref|:
  the variance (x - mean: 1, square: 1 twice over, sum: d, division: 1 -> d + 4), var + eps (1), halved by the square root: (d + 5) / 2;
  the square root, the division 1 / sqrt, x - mean, the product with r, the affine fmaf, 1 + scale, the modulation fmaf: 7; one more
  for the second-order terms:  c = ceil((d + 5) / 2) + 8.
* the ONE rounding to T: half an ulp of T at the magnitude the float32 value can have.
Worst observed ratios: profiles/normquant_accuracy.md."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))
SHAPES = [(3, 8, 8), (5, 136, 136), (64, 640, 640), (33, 1280, 1280), (7, 264, 288), (3, 4104, 4104)]  # (M, K, ldx); 4104: the sweep form


def _inputs(m, k, ldx, dtype, affine, mod, dev):
    g = torch.Generator().manual_seed(1000 * k + m)
    x = torch.randn(m, k, generator=g) * (0.25 + 4 * torch.rand(m, 1, generator=g)) + 3 * torch.randn(m, 1, generator=g)
    x[1] = 1.75                                  # a constant row: var = 0
    x[2] = x[2] * 0.01
    x[2, (5 * k) // 8] = 200.0                   # a single large outlier
    buf = torch.zeros(m, ldx, dtype=dtype, device=dev)
    buf[:, :k] = x.to(dtype)
    adt = torch.float32 if affine.endswith("32") else dtype
    w = (1 + 0.5 * torch.randn(k, generator=g)).to(adt).to(dev) if affine != "none" else None
    b = (0.5 * torch.randn(k, generator=g)).to(adt).to(dev) if affine.startswith("wb") else None
    sc = (0.3 * torch.randn(2, k, generator=g)).to(dtype).to(dev) if mod else None
    sh = (0.5 * torch.randn(2, k, generator=g)).to(dtype).to(dev) if mod else None
    return buf[:, :k], w, b, sc, sh


def _reference(x, rms, w, b, sc, sh, rows_per_batch):
    """(ref, mag, shifted) in float64: the formula, the magnitude of z's summands, what the mean's error is multiplied by."""
    f = lambda t: t.detach().cpu().to(torch.float64)  # noqa: E731
    x = f(x)
    mean = torch.zeros(x.shape[0], 1, dtype=torch.float64) if rms else x.mean(-1, keepdim=True)
    r = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + EPS)
    n = (x - mean) * r
    one = torch.ones(1, x.shape[1], dtype=torch.float64)
    w = one if w is None else f(w)[None]
    b = 0 * one if b is None else f(b)[None]
    s1 = one if sc is None else 1 + f(sc).repeat_interleave(rows_per_batch, 0)
    sh = 0 * one if sh is None else f(sh).repeat_interleave(rows_per_batch, 0)
    ref = (n * w + b) * s1 + sh
    mag = (n * w * s1).abs() + (b * s1).abs() + sh.abs()
    shifted = (0 if rms else x.abs().mean(-1, keepdim=True)) * r * (w * s1).abs()
    return ref, mag, shifted


def _half_ulp(v, dtype):
    """Half the spacing of `dtype` at magnitude v (float64 tensor), subnormal spacing below the smallest normal."""
    fi = torch.finfo(dtype)
    e = torch.floor(torch.log2(v.clamp_min(fi.tiny)))
    return 0.5 * torch.exp2(e) * fi.eps


@pytest.mark.parametrize("m, k, ldx", SHAPES)
@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mod", [False, True], ids=["plain", "adaln"])
@pytest.mark.parametrize("norm, affine", [("layer", "none"), ("layer", "w"), ("layer", "wb"), ("layer", "wb32"), ("rms", "none"), ("rms", "w")])
def test_norm_rowquant(norm, affine, mod, dtype, mm_name, m, k, ldx):
    from sdnq_amd import ops
    dev = torch.device("cuda:0")
    mm = ops.mm_code(mm_name)
    if mod and m % 2:
        m += 1  # two batches
    rms = norm == "rms"
    x, w, b, sc, sh = _inputs(m, k, ldx, dtype, affine, mod, dev)
    def call(xx, want_y=True, sc=sc, sh=sh):
        return ops.norm_rowquant(xx, ops.NORM_RMS if rms else ops.NORM_LAYER, EPS, w, b, sc, sh, mm, want_y=want_y)

    y, xq, xs = call(x)

    # 1. y against the float64 formula
    ref, mag, shifted = _reference(x, rms, w, b, sc, sh, m // 2)
    d = math.ceil(k / 512) + 9
    c = math.ceil((d + 5) / 2) + 8
    err = 2.0 ** -24 * (c * mag + (d + 1) * shifted)
    bound = _half_ulp(ref.abs() + err, dtype) + err
    ratio = ((y.cpu().to(torch.float64) - ref).abs() / bound).max().item()
    print(f"normquant accuracy {norm} {affine} {'adaln' if mod else 'plain'} {dtype} M={m} K={k}: worst |y - ref| / bound = {ratio:.4f}")
    assert torch.isfinite(y.float()).all() and ratio <= 1.0

    # 2. the codes are the row quantizer's for that y, stored or not
    def same(a, b):
        return all(torch.equal(t.view(torch.uint8), r.view(torch.uint8)) for t, r in zip(a, b))

    assert same((xq, xs), ops.rowquant(y, mm, 0)[:2])
    y0, xq0, xs0 = call(x, want_y=False)
    assert y0 is None and same((xq0, xs0), (xq, xs))

    # 3. the same bits again, and for the same rows inside a larger grid (with the modulation: one more whole batch, so a row keeps its batch)
    assert same(call(x), (y, xq, xs))
    if mod:
        padded = call(torch.cat([x, x[:m // 2].flip(0)], 0), sc=torch.cat([sc, sc[:1]], 0), sh=torch.cat([sh, sh[:1]], 0))
    else:
        padded = call(torch.cat([x, x.flip(0), x[:3]], 0))
    assert same([t[:m] for t in padded], (y, xq, xs))
