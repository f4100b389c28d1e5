"""Bit-exact GPU tests of the two adapter kernels, sdnq_hip_lowrank_add and sdnq_hip_lowrank_grad (csrc/lowrank_train.hip).

Exact-sum operands (tests/exact_inputs.py) make the float32 accumulator of every output exact in every summation order, so each output
has ONE correct bit pattern -- fma(scale, acc, y0) or scale * acc rounded once to float32, then to the stored dtype -- and the comparison
is np.array_equal on the bits (tests/lora_util.py restates both kernels in numpy).  The shapes cover ragged row and column tiles of both
kernels (64 x 128 outputs per workgroup of lowrank_add; 64 columns x one slab per workgroup of lowrank_grad), ranks that are no multiple
of the MFMA's 32 (8, 16, 40) and the slab boundary of the deterministic reduction: M below one slab, exactly one, one row more, and 4100
rows = 16 slabs and a ragged 17th.  No case is vacuous: L.add_case / L.grad_case assert on the CPU that a lost rank column / a lost
16-row block changes the stored bits of at least half of the outputs.  The one-hot census makes every output ONE product of arbitrary
finite values and so pins the element mapping: row tile, rank padding, the transposed LDS read.
"""
import numpy as np
import pytest
import torch

from sdnq_amd import ops
from tests import exact_inputs as X
from tests import lora_util as L
from tests.lowrank_util import DT, SENSITIVITY_FLOOR, bits, where

pytestmark = pytest.mark.gpu

FMTS = ("bf16", "f16")


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _same(got: np.ndarray, want: np.ndarray, *what):
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{what}: {where(got, want)}"


# ---- lowrank_add ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", L.ADD_RANKS)
@pytest.mark.parametrize("mn", L.ADD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_add_exact_sums(fmt, mn, rank, gpu_device):
    m, n = mn
    ex, y0, share = L.add_case(m, n, rank, fmt)
    assert share >= SENSITIVITY_FLOOR
    t, up = ex.a.to(gpu_device), ex.b.to(gpu_device)
    for scale in L.SCALES:
        y = torch.from_numpy(y0).to(DT[fmt]).to(gpu_device)
        assert np.array_equal(_f32(y), y0), "y0 must be values of the dtype"
        out = ops.lowrank_add(t, up, y, scale)
        assert out.data_ptr() == y.data_ptr()
        _same(_f32(y), L.add_expected(ex.acc(), y0, scale, fmt), "lowrank_add", fmt, mn, rank, scale)


@pytest.mark.parametrize("rank", (16, 40))
@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_add_two_row_tiles_per_wave(fmt, rank, gpu_device):
    """The launcher gives a wave two 16-row tiles once the launch is large; every case above runs with one."""
    m, n = L.ADD_TWO_TILES
    assert L.add_row_tiles(m, n) == 2 and all(L.add_row_tiles(*mn) == 1 for mn in L.ADD_SHAPES)
    ex, y0, share = L.add_case(m, n, rank, fmt)
    assert share >= SENSITIVITY_FLOOR
    y = torch.from_numpy(y0).to(DT[fmt]).to(gpu_device)
    ops.lowrank_add(ex.a.to(gpu_device), ex.b.to(gpu_device), y, 0.3)
    _same(_f32(y), L.add_expected(ex.acc(), y0, 0.3, fmt), "lowrank_add", fmt, (m, n), rank, "two row tiles")


@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_add_on_a_column_slice_leaves_its_surroundings(fmt, gpu_device):
    """ldy = n + 24: y is a column slice of a wider buffer with one more row behind it; the sentinels keep their bytes."""
    m, n, rank = 100, 136, 40
    ex, y0, _ = L.add_case(m, n, rank, fmt)
    wide = torch.full((m + 1, n + 24), 3.0, dtype=DT[fmt])
    wide[:m, 8:8 + n] = torch.from_numpy(y0).to(DT[fmt])
    wide = wide.to(gpu_device)
    y = wide[:m, 8:8 + n]
    assert y.stride(0) == n + 24
    ops.lowrank_add(ex.a.to(gpu_device), ex.b.to(gpu_device), y, 0.3)
    _same(_f32(y), L.add_expected(ex.acc(), y0, 0.3, fmt), "lowrank_add", fmt, "column slice")
    rest = wide.clone()
    rest[:m, 8:8 + n] = 3.0
    assert bool((rest == 3.0).all()), "bytes outside the slice changed"


@pytest.mark.parametrize("transposed", (False, True), ids=("t_one_hot", "up_one_hot"))
@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_add_rank_census(fmt, transposed, gpu_device):
    for m, n, rank in ((33, 72, 8), (100, 136, 40), (257, 264, 64)):
        for shift in X.one_hot_shifts(rank):
            t, up, want = L.add_census(m, n, rank, shift, fmt, transposed)
            y = torch.zeros((m, n), dtype=DT[fmt], device=gpu_device)
            ops.lowrank_add(t.to(gpu_device), up.to(gpu_device), y, 1.0)
            assert np.array_equal(bits(y), bits(want)), f"lowrank_add census {fmt} {(m, n, rank)} shift {shift}: {where(bits(y), bits(want))}"


# ---- lowrank_grad --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", L.GRAD_P)
@pytest.mark.parametrize("m", L.GRAD_M)
@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_grad_exact_sums(fmt, m, p, gpu_device):
    for rank in L.GRAD_RANKS:
        a, b, acc, share = L.grad_case(m, p, rank, fmt)
        assert share >= SENSITIVITY_FLOOR
        a, b = a.to(gpu_device), b.to(gpu_device)
        for tag in L.OUT_TAGS:
            want = L.grad_expected(acc, tag)
            for out_t in (False, True):
                got = ops.lowrank_grad(a, b, L.grad_scale(tag), out_t=out_t, out_dtype=DT[tag])
                assert got.dtype == DT[tag] and got.shape == ((rank, p) if out_t else (p, rank))
                _same(_f32(got), want.T if out_t else want, "lowrank_grad", fmt, (m, p, rank), tag, "out_t" if out_t else "")


@pytest.mark.parametrize("rank", L.GRAD_TILE_RANKS)
@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_grad_every_rank_tile_form(fmt, rank, gpu_device):
    """The kernel is instantiated per number of 16-column rank tiles (1, 2, 4, 8, 16: LDS row size, chunks per thread and swizzle differ);
    the ranks of test_lowrank_grad_exact_sums reach 1 and 4.  Ranks 24 / 32, 128 and 256 reach the other three, on one slab and on three."""
    assert {L.grad_rank_tiles(r) for r in L.GRAD_RANKS} == {1, 4}
    assert {L.grad_rank_tiles(r) for r in L.GRAD_TILE_RANKS} == {2, 8, 16} and L.grad_rank_tiles(rank) in (2, 8, 16)
    for m, p in L.GRAD_TILE_SHAPES:
        a, b, acc, share = L.grad_case(m, p, rank, fmt)
        assert share >= SENSITIVITY_FLOOR
        a, b = a.to(gpu_device), b.to(gpu_device)
        for tag in L.OUT_TAGS:
            want = L.grad_expected(acc, tag)
            for out_t in (False, True):
                got = ops.lowrank_grad(a, b, L.grad_scale(tag), out_t=out_t, out_dtype=DT[tag])
                _same(_f32(got), want.T if out_t else want, "lowrank_grad", fmt, (m, p, rank), tag, "out_t" if out_t else "")


@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_add_with_a_zero_sum_keeps_every_bit_of_y(fmt, gpu_device):
    """up == 0: the sum of every element is +0, and y keeps its bits -- negative zeros, subnormals and infinities included."""
    m, n, rank = 33, 72, 16
    g = torch.Generator().manual_seed(9)
    y0 = torch.randn(m, n, generator=g).to(DT[fmt])
    y0[::3, ::5] = -0.0
    y0[1, 1], y0[2, 2], y0[3, 3] = float("inf"), float("-inf"), 2.0 ** -20
    assert bool((bits(y0) == np.int16(-32768)).any())
    t = torch.randn(m, rank, generator=g).to(DT[fmt])
    y = y0.clone().to(gpu_device)
    ops.lowrank_add(t.to(gpu_device), torch.zeros(n, rank, dtype=DT[fmt], device=gpu_device), y, 0.3)
    assert np.array_equal(bits(y), bits(y0)), where(bits(y), bits(y0))


def test_lowrank_grad_default_workspace_does_not_grow_inside_a_capture(gpu_device):
    a = torch.zeros(4100, 264, dtype=torch.bfloat16, device=gpu_device)
    b = torch.zeros(4100, 256, dtype=torch.bfloat16, device=gpu_device)       # 17 slabs x 264 x 256 x 4 bytes: beyond the default megabyte
    with pytest.raises(ops._lib.SdnqHipError, match="grow inside a graph capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ops.lowrank_grad(a, b)
    torch.cuda.synchronize()
    assert not ops.lowrank_grad(a, b).any()                                    # eager: the buffer grows and the call runs


@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_grad_on_a_column_slice_twice_and_in_a_graph(fmt, gpu_device):
    """lda > P; two calls give the same bits; a captured call, workspace included, replays the eager bits."""
    m, p, rank = 4100, 264, 40
    a, b, acc, _ = L.grad_case(m, p, rank, fmt)
    wide = torch.full((m, p + 24), 3.0, dtype=DT[fmt])
    wide[:, 8:8 + p] = a
    av, b = wide.to(gpu_device)[:, 8:8 + p], b.to(gpu_device)
    assert av.stride(0) == p + 24
    want = L.grad_expected(acc, "bf16", 0.3)
    first = ops.lowrank_grad(av, b, 0.3, out_dtype=torch.bfloat16)
    _same(_f32(first), want, "lowrank_grad", fmt, "column slice")
    again = ops.lowrank_grad(av, b, 0.3, out_dtype=torch.bfloat16)
    assert np.array_equal(bits(first), bits(again)), "two calls differ"
    nbytes = ops.lowrank_grad_workspace_bytes(m, p, rank)
    assert nbytes == -(-m // L.LRG_SLAB) * p * rank * 4
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=gpu_device)
    eager = ops.lowrank_grad(av, b, 0.3, out_dtype=torch.bfloat16, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.lowrank_grad(av, b, 0.3, out_dtype=torch.bfloat16, workspace=ws)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(captured), bits(eager)) and np.array_equal(bits(eager), bits(first)), "graph replay differs"


@pytest.mark.parametrize("transposed", (False, True), ids=("a_one_hot", "b_one_hot"))
@pytest.mark.parametrize("fmt", FMTS)
def test_lowrank_grad_row_census(fmt, transposed, gpu_device):
    for m, p, rank in ((33, 72, 8), (L.LRG_SLAB + 1, 136, 40), (600, 264, 64), (L.LRG_SLAB + 1, 136, 32), (600, 72, 128), (300, 72, 256)):
        for shift in X.one_hot_shifts(m):
            a, b, prod = L.grad_census(m, p, rank, shift, fmt, transposed)
            for tag in (fmt, "f32"):
                got = ops.lowrank_grad(a.to(gpu_device), b.to(gpu_device), 1.0, out_dtype=DT[tag])
                want = torch.from_numpy(prod).to(DT[tag])
                assert np.array_equal(bits(got), bits(want)), \
                    f"lowrank_grad census {fmt}->{tag} {(m, p, rank)} shift {shift}: {where(bits(got), bits(want))}"
