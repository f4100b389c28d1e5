"""Bit-exact GPU tests of the three dropout kernels: sdnq_hip_lowrank_down_dropout (csrc/lowrank_down_kernel.h), sdnq_hip_lowrank_grad_dropout
and sdnq_hip_lowrank_add_dropout (csrc/lowrank_grad_kernel.h, csrc/lowrank_add_kernel.h).

The mask always comes from the oracle on the CPU -- oracle.adamw_halves(rows * cols, seed, offset, 5) >= T, the Philox convention the
AdamW tests pin -- never from the GPU.  Each kernel must then equal its plain sibling on the pre-masked operand bit for bit (down, grad),
or keep exactly the dropped elements (add).  The operands are exact-sum operands without a zero entry (tests/exact_inputs.py, density 1),
so a single wrong mask bit moves an exact accumulator by a nonzero product; that it also moves STORED bits is asserted on the CPU per
case: for the census of the add kernel every sum is `rank`, for grad the float32 output holds the exact accumulator, for down every
(row, k) is flipped in turn and at least one of the row's rounded outputs must change.

Shapes: the smallest that reach each path -- a ragged K stage, two rank tiles with a ragged second, both row-tile forms of the down and
add launchers, one slab / three slabs with a ragged last one and a ragged column tile of grad, row-strided operands (the mask follows
the logical index, not the stride) -- with p in {0.1, 0.5} and an offset above 2^32."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdnq_amd import lora, ops
from tests import exact_inputs as X
from tests import lora_util as L
from tests.lowrank_util import DT, bits, lrd_row_tiles, round_to, where

pytestmark = pytest.mark.gpu

FMTS = ("bf16", "f16")
STREAM = 5
# (p, seed, offset): an offset and a seed above 2^32 reach the high counter and key words
DRAWS = ((0.1, 1234, 8), (0.5, (7 << 32) + 99, (1 << 32) + 12))
DRAW_IDS = ("p0.1", "p0.5_high_words")


@functools.lru_cache(maxsize=16)
def keep_mask(rows: int, cols: int, seed: int, offset: int, thr: int) -> np.ndarray:
    """bool [rows, cols]: True where the element with logical index i * cols + j is kept."""
    return (O.adamw_halves(rows * cols, seed, offset, STREAM) >= thr).reshape(rows, cols)


def masked(x: torch.Tensor, keep: np.ndarray) -> torch.Tensor:
    return torch.where(torch.from_numpy(keep).to(x.device), x, torch.zeros((), dtype=x.dtype, device=x.device))


def same(got: torch.Tensor, want: torch.Tensor, *what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), f"{what}: {where(bits(got), bits(want))}"


def test_the_masks_differ_between_draws_and_are_not_trivial():
    for p, seed, offset in DRAWS:
        thr = lora.dropout_threshold(p)
        keep = keep_mask(40, 144, seed, offset, thr)
        share = 1.0 - float(keep.mean())
        assert abs(share - thr / 65536) < 4 * np.sqrt(p * (1 - p) / keep.size), (p, share)       # four standard deviations
        assert not np.array_equal(keep, keep_mask(40, 144, seed, offset + 1, thr))
        assert not np.array_equal(keep, keep_mask(40, 144, seed + 1, offset, thr))


# ---- the add kernel: mask census, then kept / dropped elements ---------------------------------------------------------------------------
ADD_CENSUS = ((40, 136), (8192, 1024))   # ragged on both axes; the smallest launch that takes two row tiles per wave (8 x 64 = 512)


@pytest.mark.parametrize("draw", DRAWS, ids=DRAW_IDS)
@pytest.mark.parametrize("mn", ADD_CENSUS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", FMTS)
def test_add_mask_census(fmt, mn, draw, gpu_device):
    """t = 1, up = 1, y = 0: every sum is `rank` != 0, so y != 0 exactly where the mask keeps -- every bit of the mask is read back."""
    (m, n), (p, seed, offset), rank = mn, draw, 16
    assert L.add_row_tiles(*ADD_CENSUS[0]) == 1 and L.add_row_tiles(*ADD_CENSUS[1]) == 2
    assert L.add_row_tiles(ADD_CENSUS[1][0] - 128, ADD_CENSUS[1][1]) == 1                           # ... and the smallest such M at this N
    thr = lora.dropout_threshold(p)
    keep = keep_mask(m, n, seed, offset, thr)
    dt = DT[fmt]
    t, up = torch.ones(m, rank, dtype=dt, device=gpu_device), torch.ones(n, rank, dtype=dt, device=gpu_device)
    y = torch.zeros(m, n, dtype=dt, device=gpu_device)
    out = ops.lowrank_add_dropout(t, up, y, 1.0, thr, seed, offset)
    assert out.data_ptr() == y.data_ptr()
    got = y.cpu()
    assert np.array_equal((got != 0).numpy(), keep), f"census {fmt} {mn}: {where((got != 0).numpy(), keep)}"
    assert bool((got[torch.from_numpy(keep)] == rank).all())
    y2 = torch.zeros(m, n, dtype=dt, device=gpu_device)
    ops.lowrank_add_dropout(t, up, y2, 1.0, thr, seed, offset)
    same(y2, y, "the same call twice")
    y3 = torch.zeros(m, n, dtype=dt, device=gpu_device)
    ops.lowrank_add_dropout(t, up, y3, 1.0, thr, seed, offset + 1)
    assert np.array_equal((y3.cpu() != 0).numpy(), keep_mask(m, n, seed, offset + 1, thr)) and not torch.equal(y3, y)


def _planted(y: torch.Tensor, fmt: str):
    """y with -0.0 planted on a diagonal stripe (kept and dropped elements alike), and the int16 pattern of -0.0."""
    neg0 = torch.zeros((), dtype=DT[fmt]).copy_(torch.tensor(-0.0))
    m, n = y.shape
    rows = torch.arange(0, m, 7)
    y[rows, (rows * 5) % n] = neg0
    return y, neg0.view(torch.int16).item()


def _check_add(t, up, y, scale, keep, thr, seed, offset, neg0_bits, what):
    plain = ops.lowrank_add(t, up, y.clone(), scale)
    got = ops.lowrank_add_dropout(t, up, y.clone(), scale, thr, seed, offset)
    kd = torch.from_numpy(keep).to(y.device)
    same(got, torch.where(kd, plain, y), "lowrank_add_dropout", *what)
    dropped_neg0 = (~kd) & (y.view(torch.int16) == neg0_bits)
    assert int(dropped_neg0.sum()) > 0 and bool((got.view(torch.int16)[dropped_neg0] == neg0_bits).all()), what
    assert not torch.equal(got, plain) and not torch.equal(got, y), what


@pytest.mark.parametrize("draw", DRAWS, ids=DRAW_IDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_add_keeps_the_bits_of_dropped_elements(fmt, draw, gpu_device):
    """Kept elements: the bits of plain ops.lowrank_add on a copy.  Dropped elements: their own bits, planted -0.0 included.
    t and up are exact-sum operands without a zero entry, y is random in their units (j0 2^(ea + eb), j0 in -4 .. 4, as L.add_case draws
    it) and the scale a power of two, so fma(scale, sum, y) is a float32 value that the dtype holds: ONE correct bit pattern per element."""
    (p, seed, offset), scale = draw, 0.25
    thr = lora.dropout_threshold(p)
    for (m, n), rank in ((ADD_CENSUS[0], 40), (ADD_CENSUS[1], 16)):
        keep = keep_mask(m, n, seed, offset, thr)
        if m * n <= 1 << 16:
            ex, y0, _ = L.add_case(m, n, rank, fmt)
            want = L.add_expected(ex.acc(), y0, scale, fmt)
            assert float((want != y0).mean()) > 0.9                        # on the CPU: a wrong mask bit is visible wherever the term moves y
        else:
            ex = X.exact_operands(m, n, rank, 5, fmt, density=1.0, exact_span=False)
            j0 = np.random.default_rng(6).integers(-X.IMAX, X.IMAX + 1, size=(m, n))
            y0 = (j0 * np.exp2((ex.ea[:, None] + ex.eb[None, :]).astype(np.float64))).astype(np.float32)
        assert bool((ex.a != 0).all()) and bool((ex.b != 0).all())
        y = torch.from_numpy(y0).to(DT[fmt])
        assert np.array_equal(y.float().numpy(), y0), "y0 must be values of the dtype"
        y, neg0_bits = _planted(y, fmt)
        _check_add(ex.a.to(gpu_device), ex.b.to(gpu_device), y.to(gpu_device), scale, keep, thr, seed, offset, neg0_bits, (fmt, (m, n), rank, p))


@pytest.mark.parametrize("draw", DRAWS, ids=DRAW_IDS)
def test_add_on_arbitrary_values(draw, gpu_device):
    """The same with values that are no exact sums -- y normal, scale 0.3 -- in bfloat16, at both launch forms.  Not in float16: there the
    compiler turns round_f16(fmaf(scale, sum, y)) into v_fma_mixlo_f16 (ONE rounding of the exact result) for some of a lane's 8
    elements and into v_pk_fma_f32 + v_cvt_pk_f16_f32 (two) for the others, in the plain kernel (2 of 8) as in this one (4 of 8); where
    the float32 result is not exact the two roundings differ by one float16 ulp now and then (measured against a build of this kernel that
    rounded all 8 twice: 19946 of 8388608 elements at 8192 x 1024, normal y, scale 0.3), so there "the plain kernel's bits" are the bits
    of ITS instruction choice.  bfloat16 has no such instruction; both kernels round twice everywhere."""
    (p, seed, offset), fmt = draw, "bf16"
    thr = lora.dropout_threshold(p)
    for (m, n), rank in ((ADD_CENSUS[0], 40), (ADD_CENSUS[1], 16)):
        g = torch.Generator().manual_seed(m + rank)
        t, up = (torch.randn(m, rank, generator=g) * 0.3).to(DT[fmt]), (torch.randn(n, rank, generator=g) * 0.3).to(DT[fmt])
        y, neg0_bits = _planted(torch.randn(m, n, generator=g).to(DT[fmt]), fmt)
        _check_add(t.to(gpu_device), up.to(gpu_device), y.to(gpu_device), 0.3, keep_mask(m, n, seed, offset, thr), thr, seed, offset, neg0_bits,
                   (fmt, (m, n), rank, p, "arbitrary values"))


def test_add_on_a_column_slice_follows_the_logical_index(gpu_device):
    m, n, rank, fmt = 40, 136, 16, "bf16"
    p, seed, offset = DRAWS[1]
    thr = lora.dropout_threshold(p)
    wide = torch.full((m + 1, n + 24), 3.0, dtype=DT[fmt], device=gpu_device)
    wide[:m, 8:8 + n] = 0
    y = wide[:m, 8:8 + n]
    ones = torch.ones(m, rank, dtype=DT[fmt], device=gpu_device), torch.ones(n, rank, dtype=DT[fmt], device=gpu_device)
    ops.lowrank_add_dropout(*ones, y, 1.0, thr, seed, offset)
    assert np.array_equal((y.cpu() != 0).numpy(), keep_mask(m, n, seed, offset, thr))
    rest = wide.clone()
    rest[:m, 8:8 + n] = 3.0
    assert bool((rest == 3.0).all()), "bytes outside the slice changed"


# ---- the down kernel -------------------------------------------------------------------------------------------------------------------
def down_flips_are_visible(ex: X.Exact, keep: np.ndarray, fmt: str, rows: np.ndarray) -> bool:
    """On the CPU: flip the mask bit of every (row, k) of `rows` in turn; at least one of the row's R rounded outputs must change."""
    ia, mk = ex.ia[rows], keep[rows]
    base = X.int_matmul(ia * mk, ex.ib)                                                  # [rows, R] exact integer accumulators
    delta = ia[:, :, None] * ex.ib.T[None, :, :]                                         # [rows, K, R]: what element (row, k) contributes
    flipped = base[:, None, :] + np.where(mk, -1, 1)[:, :, None] * delta
    unit = np.exp2((ex.ea[rows, None] + ex.eb[None, :]).astype(np.float64))
    rb = round_to(base * unit, fmt)
    rf = round_to((flipped * unit[:, None, :]).reshape(-1, unit.shape[1]), fmt).reshape(flipped.shape)
    return bool((rf != rb[:, None, :]).any(-1).all())


DOWN_CASES = ((40, 144, 8), (40, 144, 16), (40, 144, 40), (4112, 144, 16))   # K = one full stage + a partial one; rank 40: two rank tiles


@pytest.mark.parametrize("draw", DRAWS, ids=DRAW_IDS)
@pytest.mark.parametrize("mkr", DOWN_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", FMTS)
def test_down_equals_the_plain_kernel_on_the_masked_input(fmt, mkr, draw, gpu_device):
    (m, k, r), (p, seed, offset) = mkr, draw
    assert lrd_row_tiles(40) == 1 and lrd_row_tiles(4112) == 2 and lrd_row_tiles(4112 - 16) == 1   # the smallest M class with two row tiles
    thr = lora.dropout_threshold(p)
    ex = X.exact_operands(m, r, k, 17 + m + 3 * k + r, fmt, density=1.0)
    assert bool((ex.a != 0).all()) and bool((ex.b != 0).all()) and ex.span_bits <= X.B[L.MFMA[fmt]]
    keep = keep_mask(m, k, seed, offset, thr)
    rows = np.arange(m) if m <= 64 else np.r_[0:16, m // 2:m // 2 + 16, m - 16:m]
    assert down_flips_are_visible(ex, keep, fmt, rows)
    x, down = ex.a.to(gpu_device), ex.b.to(gpu_device)
    want = ops.lowrank_down(masked(x, keep), down)
    got = ops.lowrank_down_dropout(x, down, thr, seed, offset)
    same(got, want, "lowrank_down_dropout", fmt, mkr, p)
    # ... which is the CPU's value too: the exact sums of the masked operand, rounded once
    unit = np.exp2((ex.ea[:, None] + ex.eb[None, :]).astype(np.float64))
    assert np.array_equal(got.float().cpu().numpy(), round_to(X.int_matmul(ex.ia * keep, ex.ib) * unit, fmt))
    same(ops.lowrank_down_dropout(x, down, thr, seed, offset), got, "the same call twice")
    assert not torch.equal(ops.lowrank_down_dropout(x, down, thr, seed, offset + 1), got)
    assert not torch.equal(ops.lowrank_down(x, down), got)


@pytest.mark.parametrize("fmt", FMTS)
def test_down_on_a_row_strided_input_follows_the_logical_index(fmt, gpu_device):
    m, k, r = 40, 144, 16
    p, seed, offset = DRAWS[1]
    thr = lora.dropout_threshold(p)
    ex = X.exact_operands(m, r, k, 17 + m + 3 * k + r, fmt, density=1.0)
    keep = keep_mask(m, k, seed, offset, thr)
    wide = torch.full((m, k + 16), 3.0, dtype=DT[fmt])
    wide[:, :k] = ex.a
    x = wide.to(gpu_device)[:, :k]
    assert x.stride(0) == k + 16
    got = ops.lowrank_down_dropout(x, ex.b.to(gpu_device), thr, seed, offset)
    same(got, ops.lowrank_down(masked(ex.a.to(gpu_device), keep), ex.b.to(gpu_device)), "row-strided x", fmt)
    same(got, ops.lowrank_down_dropout(ex.a.to(gpu_device), ex.b.to(gpu_device), thr, seed, offset), "strided against contiguous", fmt)


# ---- the grad kernel -------------------------------------------------------------------------------------------------------------------
GRAD_CASES = ((200, 72, 16), (200, 72, 64), (675, 72, 16), (675, 72, 64))   # one slab, direct store / three slabs, the last ragged; P = 72


@pytest.mark.parametrize("draw", DRAWS, ids=DRAW_IDS)
@pytest.mark.parametrize("mpr", GRAD_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", FMTS)
def test_grad_equals_the_plain_kernel_on_the_masked_operand(fmt, mpr, draw, gpu_device):
    (m, pcols, r), (p, seed, offset) = mpr, draw
    assert -(-200 // L.LRG_SLAB) == 1 and -(-675 // L.LRG_SLAB) == 3 and 675 % L.LRG_SLAB and pcols % 64
    thr = lora.dropout_threshold(p)
    a, b, acc, _ = L.grad_case(m, pcols, r, fmt)
    assert bool((a != 0).all()) and bool((b != 0).all())
    # on the CPU: flipping the bit of (i, j) moves the exact accumulators of out[j][:] by a[i][j] b[i][:] != 0, and the float32 output
    # with scale 1 IS the accumulator (it fits the float32 significand: grad_case holds the span to the measured budget)
    assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
    keep = keep_mask(m, pcols, seed, offset, thr)
    a, b = a.to(gpu_device), b.to(gpu_device)
    am = masked(a, keep)
    for out_t in (False, True):
        got32 = ops.lowrank_grad_dropout(a, b, 1.0, thr, seed, offset, out_t=out_t, out_dtype=torch.float32)
        same(got32, ops.lowrank_grad(am, b, 1.0, out_t=out_t, out_dtype=torch.float32), "lowrank_grad_dropout f32", fmt, mpr, out_t)
        exact = (a.double().cpu().numpy() * keep).T @ b.double().cpu().numpy()
        assert np.array_equal(got32.double().cpu().numpy(), exact.T if out_t else exact)
        got = ops.lowrank_grad_dropout(a, b, 0.3, thr, seed, offset, out_t=out_t)
        same(got, ops.lowrank_grad(am, b, 0.3, out_t=out_t), "lowrank_grad_dropout", fmt, mpr, out_t)
        assert got.shape == ((r, pcols) if out_t else (pcols, r)) and got.dtype == DT[fmt]
    same(ops.lowrank_grad_dropout(a, b, 1.0, thr, seed, offset, out_dtype=torch.float32),
         ops.lowrank_grad_dropout(a, b, 1.0, thr, seed, offset, out_dtype=torch.float32), "the same call twice")
    assert not torch.equal(ops.lowrank_grad_dropout(a, b, 1.0, thr, seed, offset + 1, out_dtype=torch.float32),
                           ops.lowrank_grad_dropout(a, b, 1.0, thr, seed, offset, out_dtype=torch.float32))


@pytest.mark.parametrize("fmt", FMTS)
def test_grad_on_a_row_strided_operand_follows_the_logical_index(fmt, gpu_device):
    m, pcols, r = 675, 72, 16
    p, seed, offset = DRAWS[1]
    thr = lora.dropout_threshold(p)
    a, b, _, _ = L.grad_case(m, pcols, r, fmt)
    keep = keep_mask(m, pcols, seed, offset, thr)
    wide = torch.full((m, pcols + 24), 3.0, dtype=DT[fmt])
    wide[:, 8:8 + pcols] = a
    av = wide.to(gpu_device)[:, 8:8 + pcols]
    assert av.stride(0) == pcols + 24
    b = b.to(gpu_device)
    got = ops.lowrank_grad_dropout(av, b, 1.0, thr, seed, offset, out_t=True, out_dtype=torch.float32)
    same(got, ops.lowrank_grad(masked(a.to(gpu_device), keep), b, 1.0, out_t=True, out_dtype=torch.float32), "row-strided a", fmt)
