"""Inputs and CPU expected values of the conv adapter kernels' bit-exact tests (tests/test_conv_lora_exact_gpu.py,
tests/test_conv_lora_host.py): sdnq_hip_conv_lowrank_down and sdnq_hip_conv_lowrank_grad, restated in numpy on an F.unfold restatement.

    conv_lowrank_down   t = round_dtype( f32(acc) )                  acc = unfold(x) . down^T
    conv_lowrank_grad   out = round_out( f32(scale) * f32(acc) )     acc = g^T . unfold(x), exact whatever the slabs

An element of x feeds many rows of unfold(x), so the per-row exponents of tests/exact_inputs.py do not apply: x holds nonzero integers
+-1 .. +-4 times ONE power of two, down (for the grad kernel g) nonzero integers +-1 .. +-4 times a power of two per rank column.  Every
partial sum is an integer below 16 K (16 M) units -- inside 2^20 for every case here -- so the float32 sum is exact in every order and each
output has ONE correct bit pattern.  The exponent windows keep every output a finite normal value of float16.
"""
import functools
import os
import re

import numpy as np
import torch

from tests import exact_inputs as X
from tests.lowrank_util import DT, SENSITIVITY_FLOOR

CLG_SLAB = 256   # output positions per partial sum of sdnq_hip_conv_lowrank_grad: CLG_SLAB of csrc/conv_lowrank.hip
X_EXP = (-4, 0)      # the one exponent of x
R_EXP = (-6, -1)     # the exponents of the rank columns
OUT_TAGS = ("f32", "bf16", "f16")

# name: (kernel, batch, channels, (H, W), stride, padding, dilation); Conv1d is the H = kh = 1 problem
GEOMETRIES = {
    "g1_3x3_ragged": ((3, 3), 2, 16, (7, 9), (1, 1), (1, 1), (1, 1)),        # M = 126: a 64-position block crosses the image boundary
    "g2_3x3_stride2": ((3, 3), 1, 32, (9, 11), (2, 2), (1, 1), (1, 1)),
    "g3_3x3_dilated": ((3, 3), 2, 16, (8, 8), (1, 1), (2, 2), (2, 2)),
    "g4_1x1": ((1, 1), 2, 64, (6, 6), (1, 1), (0, 0), (1, 1)),
    "g5_conv1d_k5": ((1, 5), 3, 16, (1, 37), (1, 2), (0, 2), (1, 1)),
    "g6_1x3": ((1, 3), 1, 48, (10, 7), (1, 1), (0, 1), (1, 1)),
    "g7_3x2_mixed": ((3, 2), 1, 8, (12, 10), (2, 1), (1, 0), (1, 2)),        # K = 48: one ragged K chunk
    "g8_3x3_k2880": ((3, 3), 1, 320, (16, 16), (1, 1), (1, 1), (1, 1)),      # 45 K chunks, 4 workgroups (down) / 45 column tiles (grad)
}
DOWN_RANKS = {"g1_3x3_ragged": (8, 40), "g2_3x3_stride2": (16,), "g3_3x3_dilated": (64,), "g4_1x1": (256,), "g5_conv1d_k5": (8,),
              "g6_1x3": (40, 128), "g7_3x2_mixed": (16,), "g8_3x3_k2880": (16, 64)}
# the grad kernel alone: M = 675 = two slabs and a ragged third
GRAD_GEOMETRIES = {**GEOMETRIES, "g9_3x3_three_slabs": ((3, 3), 3, 16, (15, 15), (1, 1), (1, 1), (1, 1))}
GRAD_RANKS = {**DOWN_RANKS, "g9_3x3_three_slabs": (8, 64)}


def slab_constant_in_source() -> int:
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sdnq_amd", "csrc", "conv_lowrank.hip")
    with open(src) as f:
        return int(re.search(r"constexpr int CLG_SLAB = (\d+);", f.read()).group(1))


def out_hw(geo):
    (kh, kw), _, _, (h, w), (sh, sw), (ph, pw), (dh, dw) = geo
    return (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def sizes(geo):
    """(M, K) of the unfolded matrix."""
    (kh, kw), b, c, _, _, _, _ = geo
    ho, wo = out_hw(geo)
    return b * ho * wo, c * kh * kw


def unfold(x: np.ndarray, geo) -> np.ndarray:
    """F.unfold(x, kernel, dilation, padding, stride).transpose(1, 2) flattened: [B H_out W_out][C kh kw], rows (b, oh, ow), columns
    (c, i, j), zeros outside the image."""
    (kh, kw), b, c, (h, w), (sh, sw), (ph, pw), (dh, dw) = geo
    assert x.shape == (b, c, h, w)
    ho, wo = out_hw(geo)
    xp = np.zeros((b, c, h + 2 * ph, w + 2 * pw), dtype=x.dtype)
    xp[:, :, ph:ph + h, pw:pw + w] = x
    cols = np.empty((b, c, kh, kw, ho, wo), dtype=x.dtype)
    for i in range(kh):
        for j in range(kw):
            cols[:, :, i, j] = xp[:, :, i * dh:i * dh + (ho - 1) * sh + 1:sh, j * dw:j * dw + (wo - 1) * sw + 1:sw]
    return np.ascontiguousarray(cols.transpose(0, 4, 5, 1, 2, 3)).reshape(b * ho * wo, c * kh * kw)


def inside(geo) -> np.ndarray:
    """[M][K] bool: the tap of column k lies inside the image at row m."""
    _, b, c, (h, w), _, _, _ = geo
    return unfold(np.ones((b, c, h, w), dtype=np.int64), geo) != 0


def round_f32_to(a32: np.ndarray, tag: str) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(DT[tag]).float().numpy()


def _ints(rng, shape) -> np.ndarray:
    return (rng.integers(1, X.IMAX + 1, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)).astype(np.int64)


def _f32_exact(a: np.ndarray) -> np.ndarray:
    a32 = a.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a), "accumulators must be float32 values"
    return a32


def _as(vals: np.ndarray, fmt: str) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(DT[fmt])
    assert np.array_equal(t.float().numpy().astype(np.float64), vals), "inputs must be values of the dtype"
    return t


# ---- conv_lowrank_down -----------------------------------------------------------------------------------------------------------------
def down_expected(acc: np.ndarray, fmt: str) -> np.ndarray:
    return round_f32_to(_f32_exact(acc), fmt)


def down_sensitivity(ux: np.ndarray, idown: np.ndarray, unit: np.ndarray, geo, fmt: str) -> float:
    """Drop ONE tap (i, j) -- all its channels -- or ONE input channel -- all its taps -- from the expected sum: the smallest share, over
    the taps and channels, of the stored outputs the dropped term reaches (a tap: the rows where it lies inside the image; a channel:
    every row) whose bits change."""
    (kh, kw), _, c, _, _, _, _ = geo
    kprod = kh * kw
    ints = ux @ idown.T
    out0 = down_expected(ints * unit, fmt)
    ins = inside(geo)
    worst = 1.0
    groups = [(np.arange(c) * kprod + p, ins[:, p]) for p in range(kprod)] + [(ch * kprod + np.arange(kprod), None) for ch in range(c)]
    for cols, rows in groups:
        out_c = down_expected((ints - ux[:, cols] @ idown[:, cols].T) * unit, fmt)
        changed = out_c != out0
        if rows is not None:
            if not rows.any():
                continue
            changed = changed[rows]
        worst = min(worst, float(changed.mean()))
    return worst


@functools.lru_cache(maxsize=4)
def down_case(name: str, rank: int, fmt: str):
    """(x [B, C, H, W], down [rank, K] in the dtype; the expected t as float32; the sensitivity).  Draws again (4 seeds) until the
    sensitivity reaches SENSITIVITY_FLOOR, then raises."""
    geo = GEOMETRIES[name]
    _, b, c, (h, w), _, _, _ = geo
    m, k = sizes(geo)
    assert 16 * k < 2 ** 20
    why = ""
    for attempt in range(4):
        rng = np.random.default_rng(101 + 1000 * attempt + 7 * rank + sum(map(ord, name)))
        ix, idown = _ints(rng, (b, c, h, w)), _ints(rng, (rank, k))
        ex, er = int(rng.integers(X_EXP[0], X_EXP[1] + 1)), rng.integers(R_EXP[0], R_EXP[1] + 1, size=rank)
        unit = np.exp2((ex + er).astype(np.float64))[None, :]
        ux = unfold(ix, geo)
        share = down_sensitivity(ux, idown, unit, geo, fmt)
        if share >= SENSITIVITY_FLOOR:
            x = _as(ix * np.exp2(float(ex)), fmt)
            down = _as(idown * np.exp2(er.astype(np.float64))[:, None], fmt)
            return x, down, down_expected((ux @ idown.T) * unit, fmt), share
        why = f"a lost tap or channel leaves {1 - share:.2f} of the stored outputs it reaches as they were"
    raise ValueError(f"down_case({name}, rank {rank}, {fmt}): {why}")


# ---- conv_lowrank_grad -----------------------------------------------------------------------------------------------------------------
def grad_scale(tag: str) -> float:
    return {"f32": 0.3, "bf16": 1.0, "f16": 0.25}[tag]


def grad_expected(acc: np.ndarray, tag: str, scale=None) -> np.ndarray:
    return round_f32_to(np.float32(grad_scale(tag) if scale is None else scale) * _f32_exact(acc), tag)


def grad_sensitivity(ux: np.ndarray, ig: np.ndarray, unit: np.ndarray, tag: str) -> float:
    """Drop ONE block of 16 consecutive output positions from the sum: the smallest share, over the blocks, of the stored outputs whose
    bits change (counted over all outputs, those of taps the block never reaches included)."""
    ints = ig.T @ ux
    out0 = grad_expected(ints * unit, tag)
    worst = 1.0
    for m0 in range(0, ux.shape[0], 16):
        lost = ig[m0:m0 + 16].T @ ux[m0:m0 + 16]
        worst = min(worst, float((grad_expected((ints - lost) * unit, tag) != out0).mean()))
    return worst


@functools.lru_cache(maxsize=4)
def grad_case(name: str, rank: int, fmt: str):
    """(x [B, C, H, W], g [M, rank] in the dtype; the exact accumulators [rank, K] as float64; the smallest sensitivity over OUT_TAGS)."""
    geo = GRAD_GEOMETRIES[name]
    _, b, c, (h, w), _, _, _ = geo
    m, k = sizes(geo)
    assert 16 * m < 2 ** 20
    why = ""
    for attempt in range(4):
        rng = np.random.default_rng(211 + 1000 * attempt + 7 * rank + sum(map(ord, name)))
        ix, ig = _ints(rng, (b, c, h, w)), _ints(rng, (m, rank))
        ex, er = int(rng.integers(X_EXP[0], X_EXP[1] + 1)), rng.integers(R_EXP[0], R_EXP[1] + 1, size=rank)
        unit = np.exp2((ex + er).astype(np.float64))[:, None]
        ux = unfold(ix, geo)
        share = min(grad_sensitivity(ux, ig, unit, tag) for tag in OUT_TAGS)
        if share >= SENSITIVITY_FLOOR:
            x = _as(ix * np.exp2(float(ex)), fmt)
            g = _as(ig * np.exp2(er.astype(np.float64))[None, :], fmt)
            return x, g, (ig.T @ ux) * unit, share
        why = f"a lost block of 16 positions leaves {1 - share:.2f} of the stored outputs as they were"
    raise ValueError(f"grad_case({name}, rank {rank}, {fmt}): {why}")


# ---- one product per output ------------------------------------------------------------------------------------------------------------
def census_pixels(geo):
    """(b, c, h, w) of the planted pixels: the four corners, an edge pixel, an interior pixel, a pixel of the last image."""
    _, b, c, (h, w), _, _, _ = geo
    return ((0, 0, 0, 0), (0, c - 1, 0, w - 1), (0, 1 % c, h - 1, 0), (0, c // 2, h - 1, w - 1), (0, 2 % c, h // 2, 0),
            (0, c - 1, h // 2, w // 2), (b - 1, c // 3, h // 3, (2 * w) // 3))


def down_census(name: str, pixel, rank: int, fmt: str):
    """(x with a single 1.0 at `pixel`, arbitrary down [rank, K], the expected t in the dtype): t is down[r][c0][i][j] at exactly the
    (position, tap) pairs that reach the pixel and +0 elsewhere."""
    geo = GEOMETRIES[name]
    _, b, c, (h, w), _, _, _ = geo
    m, k = sizes(geo)
    rng = np.random.default_rng(17 + sum(pixel) + sum(map(ord, name)))
    down = X._arbitrary(rng, (rank, k), fmt)
    x = np.zeros((b, c, h, w), dtype=np.float64)
    x[pixel] = 1.0
    ux = unfold(x, geo)
    assert ux.sum(axis=1).max() <= 1.0, "a position reaches a pixel through one tap at most"
    want = ux @ down.double().numpy().T + 0.0
    return _as(x, fmt), down, torch.from_numpy(want.astype(np.float32)).to(DT[fmt]), int(ux.sum())


def grad_census(name: str, row: int, rank: int, fmt: str):
    """(arbitrary x, g nonzero in row `row` alone, the expected float32 out [rank, K] at scale 1): every output is ONE product
    g[row][r] * unfold(x)[row][k], or 0 where the tap leaves the image."""
    geo = GRAD_GEOMETRIES[name]
    _, b, c, (h, w), _, _, _ = geo
    m, k = sizes(geo)
    rng = np.random.default_rng(29 + row + sum(map(ord, name)))
    x = X._arbitrary(rng, (b, c, h, w), fmt)
    g = torch.zeros((m, rank), dtype=DT[fmt])
    g[row] = X._arbitrary(rng, (rank,), fmt)
    prod = np.outer(g[row].double().numpy(), unfold(x.double().numpy(), geo)[row]) + 0.0
    return x, g, _f32_exact(prod)
