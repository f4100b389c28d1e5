"""Inputs and CPU expected values of the adapter kernels' bit-exact tests (tests/test_lora_exact_gpu.py, tests/test_lora_host.py):
sdnq_hip_lowrank_add and sdnq_hip_lowrank_grad on exact-sum operands (tests/exact_inputs.py), restated in numpy.

    lowrank_add    y = round_dtype( fma_f32(scale, acc, y0) )       acc = t . up^T, exact in float32 in every summation order
    lowrank_grad   out = round_out( f32(scale) * f32(acc) )         acc = a^T . b, exact whatever the slabs

The operands are dense (density 1.0): every product is a nonzero integer in the units of its output, so a rank column or a block of rows
that went missing moves every exact sum -- whether the STORED bits move as well is what add_sensitivity / grad_sensitivity measure, on
the CPU, from the inputs alone.
"""
import functools
import os
import re

import numpy as np
import torch

from tests import exact_inputs as X
from tests import lowrank_util as L

LRG_SLAB = 256   # rows per partial sum of sdnq_hip_lowrank_grad: LRG_SLAB of csrc/lowrank_train.hip (test_lora_host.py compares the two)
MFMA = {"bf16": "bf16_16x16x32", "f16": "f16_16x16x32"}   # keys of X.MEASURED_SPAN_BITS / X.B: both kernels run v_mfma_f32_16x16x32

ADD_SHAPES = ((5, 16), (33, 72), (257, 264), (513, 1288), (100, 136))
ADD_RANKS = (8, 16, 40, 64, 256)
ADD_TWO_TILES = (1031, 8328)   # the smallest kind of launch that takes two row tiles per wave (add_row_tiles), ragged on both axes
SCALES = (1.0, 0.25, 0.3)
GRAD_M = (5, 33, LRG_SLAB, LRG_SLAB + 1, 4100)
GRAD_P = (16, 72, 264, 1288)
GRAD_RANKS = (8, 16, 40, 64)
OUT_TAGS = ("f32", "bf16", "f16")
# ranks that reach the other rank-tile forms of sdnq_hip_lowrank_grad (grad_rank_tiles: GRAD_RANKS reach 1 and 4 tiles only), and the
# (M, P) they run at: one slab, and three slabs with a ragged last one; 264 columns = four 64-column tiles and a ragged fifth
GRAD_TILE_RANKS = (24, 32, 128, 256)
GRAD_TILE_SHAPES = ((33, 264), (600, 264))


def slab_constant_in_source() -> int:
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sdnq_amd", "csrc", "lowrank_train.hip")
    with open(src) as f:
        return int(re.search(r"constexpr int LRG_SLAB = (\d+);", f.read()).group(1))


def round_f32_to(a32: np.ndarray, tag: str) -> np.ndarray:
    """float32 values rounded to `tag` (the kernel's own second step), as float32."""
    return torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(L.DT[tag]).float().numpy()


# ---- lowrank_add -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def add_case(m: int, n: int, rank: int, fmt: str):
    """(exact-sum t [m, rank] and up [n, rank]; y0 [m, n] float32 = j0 * 2^(ea[i] + eb[j]), j0 in {0, +-1 .. +-4}; the smallest
    sensitivity over SCALES).  Draws again (4 seeds) until dropping any rank column changes at least SENSITIVITY_FLOOR of the stored
    outputs, then raises."""
    why = ""
    for attempt in range(4):
        seed = 7 + 1000 * attempt + m + 3 * n + 5 * rank
        ex = X.exact_operands(m, n, rank, seed, fmt, density=1.0)
        assert ex.span_bits <= X.B[MFMA[fmt]]
        rng = np.random.default_rng(seed + 1)
        j0 = rng.integers(-X.IMAX, X.IMAX + 1, size=(m, n))
        top = int(X.expected_int(np.abs(ex.ia), np.abs(ex.ib)).max()) + X.IMAX
        assert top < 2 ** 24, "accumulator + y0 would leave the float32 significand"
        y0 = (j0 * np.exp2((ex.ea[:, None] + ex.eb[None, :]).astype(np.float64))).astype(np.float32)
        share = min(add_sensitivity(ex, y0, s, fmt) for s in SCALES)
        if share >= L.SENSITIVITY_FLOOR:
            return ex, y0, share
        why = f"a lost rank column leaves {1 - share:.2f} of the stored outputs as they were"
    raise ValueError(f"add_case({m}, {n}, rank {rank}, {fmt}): {why}")


def add_row_tiles(m: int, n: int) -> int:
    """sdnq_hip_lowrank_add: 16-row tiles per wave -- two once workgroups of 128 rows x 128 columns still number 512."""
    return 2 if -(-n // 128) * -(-m // 128) >= 512 else 1


def add_expected(acc: np.ndarray, y0: np.ndarray, scale: float, fmt: str) -> np.ndarray:
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc), "accumulators must be float32 values"
    return round_f32_to(X._fma_f32(a32, np.full(a32.shape, scale, dtype=np.float32), y0), fmt)


def add_sensitivity(ex: X.Exact, y0: np.ndarray, scale: float, fmt: str) -> float:
    """Drop ONE rank column of the operands: the smallest share, over the columns, of the (sampled) outputs whose stored bits change."""
    m, n, rank = ex.ia.shape[0], ex.ib.shape[0], ex.ia.shape[1]
    rows = L.sample_rows(m, n, rank)
    rows = np.arange(m) if rows is None else rows
    unit = np.exp2((ex.ea[rows, None] + ex.eb[None, :]).astype(np.float64))
    ints = X.expected_int(ex.ia[rows], ex.ib)
    out0 = add_expected(ints * unit, y0[rows], scale, fmt)
    worst = 1.0
    for c in range(rank):
        out_c = add_expected((ints - ex.ia[rows, c:c + 1] * ex.ib[:, c][None, :]) * unit, y0[rows], scale, fmt)
        worst = min(worst, float((out_c != out0).mean()))
    return worst


# ---- lowrank_grad ----------------------------------------------------------------------------------------------------------------------
def grad_scale(tag: str) -> float:
    return {"f32": 0.3, "bf16": 1.0, "f16": 0.25}[tag]


def grad_rank_tiles(rank: int) -> int:
    """sdnq_hip_lowrank_grad: the 16-column rank tiles of the kernel instantiation a rank takes (its LDS row is 32 bytes per tile)."""
    return next(t for t in (1, 2, 4, 8, 16) if rank <= 16 * t)


@functools.lru_cache(maxsize=8)
def grad_case(m: int, p: int, rank: int, fmt: str):
    """(a [m, p], b [m, rank] in the dtype, the exact accumulators [p, rank] as float64, the smallest sensitivity over OUT_TAGS): the
    operands of X.exact_operands(p, rank, m), transposed."""
    why = ""
    for attempt in range(4):
        ex = X.exact_operands(p, rank, m, 11 + 1000 * attempt + m + 3 * p + 5 * rank, fmt, density=1.0)
        assert ex.span_bits <= X.B[MFMA[fmt]]
        share = min(grad_sensitivity(ex, tag) for tag in OUT_TAGS)
        if share >= L.SENSITIVITY_FLOOR:
            return ex.a.t().contiguous(), ex.b.t().contiguous(), ex.acc(), share
        why = f"a lost 16-row block leaves {1 - share:.2f} of the stored outputs as they were"
    raise ValueError(f"grad_case({m}, {p}, rank {rank}, {fmt}): {why}")


def grad_expected(acc: np.ndarray, tag: str, scale=None) -> np.ndarray:
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc), "accumulators must be float32 values"
    return round_f32_to(np.float32(grad_scale(tag) if scale is None else scale) * a32, tag)


def grad_sensitivity(ex: X.Exact, tag: str) -> float:
    """Drop ONE block of 16 consecutive rows of both operands (rows 16 k .. 16 k + 15 of the reduction): the smallest share, over the
    blocks, of the (sampled) outputs whose stored bits change."""
    p, rank, m = ex.ia.shape[0], ex.ib.shape[0], ex.ia.shape[1]
    blocks = -(-m // 16)
    rows = L.sample_rows(p, rank, blocks)
    rows = np.arange(p) if rows is None else rows
    unit = np.exp2((ex.ea[rows, None] + ex.eb[None, :]).astype(np.float64))
    ints = X.expected_int(ex.ia[rows], ex.ib)
    out0 = grad_expected(ints * unit, tag)
    worst = 1.0
    for k in range(blocks):
        lost = X.int_matmul(ex.ia[rows, 16 * k:16 * k + 16], ex.ib[:, 16 * k:16 * k + 16])
        worst = min(worst, float((grad_expected((ints - lost) * unit, tag) != out0).mean()))
    return worst


# ---- one product per output ------------------------------------------------------------------------------------------------------------
def add_census(m: int, n: int, rank: int, shift: int, fmt: str, transposed: bool):
    """(t, up, expected y from y0 = 0 and scale 1, in the dtype): the rows of t are one-hot (transposed: those of up)."""
    oh = X.one_hot_operands(n, m, rank, shift, fmt, seed=3) if transposed else X.one_hot_operands(m, n, rank, shift, fmt, seed=3)
    acc = oh.acc().T if transposed else oh.acc()
    t, up = (oh.b, oh.a) if transposed else (oh.a, oh.b)
    return t, up, torch.from_numpy(np.ascontiguousarray(acc.astype(np.float32))).to(L.DT[fmt])


def grad_census(m: int, p: int, rank: int, shift: int, fmt: str, transposed: bool):
    """(a [m, p], b [m, rank], the products [p, rank] as float32): every column of a has ONE nonzero, at row (3 j + shift) % m
    (transposed: every column of b), the other operand is dense and arbitrary."""
    oh = X.one_hot_operands(rank, p, m, shift, fmt, seed=5) if transposed else X.one_hot_operands(p, rank, m, shift, fmt, seed=5)
    acc = oh.acc().T if transposed else oh.acc()
    a, b = (oh.b, oh.a) if transposed else (oh.a, oh.b)
    return a.t().contiguous(), b.t().contiguous(), np.ascontiguousarray(acc.astype(np.float32))


# ---- end to end: the bound of tests/test_lora_gpu.py -----------------------------------------------------------------------------------
def ulp(e: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """The spacing of `dtype` at |e| (float64): 2^(floor(log2 |e|) - mantissa bits), at least the subnormal spacing."""
    bits, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}[dtype]
    ex = np.floor(np.log2(np.maximum(np.abs(e), np.exp2(float(emin)))))
    return np.exp2(np.maximum(ex, emin) - bits)


def bound(e: np.ndarray, s: np.ndarray, terms: int, dtype: torch.dtype) -> np.ndarray:
    """|got - e| <= ulp_d(e) / 2 + (L + 2) 2^-24 S: one rounding of the float32 result to the stored dtype, and the float32 arithmetic in
    front of it -- a sum of L products in any order (each partial sum within 2^-24 of S relative, L of them), the scale and the base
    value's addition (2 more)."""
    return 0.5 * ulp(e, dtype) + (terms + 2) * 2.0 ** -24 * s
