"""Bit-exact GPU tests of the two conv adapter kernels, sdnq_hip_conv_lowrank_down and sdnq_hip_conv_lowrank_grad (csrc/conv_lowrank.hip).

The inputs of tests/conv_lora_util.py make the float32 accumulator of every output exact in every summation order, so each output has
ONE correct bit pattern -- the numpy F.unfold restatement rounded once -- and the comparison is np.array_equal on the bits.  The
geometries cover a 64-position block that crosses the image boundary and is ragged (M = 126), strides, dilation, 1 x 1, Conv1d, kernels
that are not square, a ragged K chunk (K = 48), many K chunks and several workgroups (K = 2880), and for the grad kernel two slabs and a
ragged third (M = 675); ranks 8, 16, 40, 64, 128 and 256 -- and the census' 24 -- reach every rank-tile form.  No case is vacuous: C.down_case / C.grad_case
assert on the CPU that a lost tap, a lost input channel or a lost block of 16 positions changes the stored bits of at least half of the
outputs it reaches.  The census makes every output ONE product of arbitrary finite values and so pins the element mapping: which
(position, tap) pairs reach a pixel, the padding, the transposed LDS read.
"""
import numpy as np
import pytest
import torch

from sdnq_amd import ops
from tests import conv_lora_util as C
from tests.lowrank_util import DT, SENSITIVITY_FLOOR, bits, where

pytestmark = pytest.mark.gpu

FMTS = ("bf16", "f16")


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _same(got: np.ndarray, want: np.ndarray, *what):
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), f"{what}: {where(got, want)}"


def _args(geo):
    kernel, _, _, _, stride, padding, dilation = geo
    return kernel, stride, padding, dilation


def test_the_slab_constant_and_the_geometries():
    assert C.slab_constant_in_source() == C.CLG_SLAB
    assert C.sizes(C.GEOMETRIES["g1_3x3_ragged"]) == (126, 144) and C.sizes(C.GEOMETRIES["g7_3x2_mixed"])[1] == 48
    assert C.sizes(C.GEOMETRIES["g8_3x3_k2880"]) == (256, 2880) and C.sizes(C.GRAD_GEOMETRIES["g9_3x3_three_slabs"])[0] == 675
    assert {r for rs in C.DOWN_RANKS.values() for r in rs} == {8, 16, 40, 64, 128, 256}


# ---- conv_lowrank_down ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.GEOMETRIES))
@pytest.mark.parametrize("fmt", FMTS)
def test_conv_lowrank_down_exact_sums(fmt, name, gpu_device):
    geo = C.GEOMETRIES[name]
    for rank in C.DOWN_RANKS[name]:
        x, down, want, share = C.down_case(name, rank, fmt)
        print(name, rank, fmt, "sensitivity", share)
        assert share >= SENSITIVITY_FLOOR
        xg, dg = x.to(gpu_device), down.to(gpu_device)
        t, (b, ho, wo) = ops.conv_lowrank_down(xg, dg, *_args(geo))
        assert (b, ho, wo) == (geo[1], *C.out_hw(geo)) and t.shape == (b * ho * wo, rank) and t.dtype == DT[fmt]
        _same(_f32(t), want, "conv_lowrank_down", fmt, name, rank)
        # the composition it replaces: identical wherever the float32 sums are exact
        u, _ = ops.im2col(xg, *_args(geo))
        assert np.array_equal(bits(ops.lowrank_down(u, dg)), bits(t)), ("im2col + lowrank_down", fmt, name, rank)


@pytest.mark.parametrize("name", ("g1_3x3_ragged", "g2_3x3_stride2", "g3_3x3_dilated", "g5_conv1d_k5", "g7_3x2_mixed"))
@pytest.mark.parametrize("fmt", FMTS)
def test_conv_lowrank_down_pixel_census(fmt, name, gpu_device):
    geo = C.GEOMETRIES[name]
    for pixel in C.census_pixels(geo):
        x, down, want, reached = C.down_census(name, pixel, 24, fmt)
        assert reached > 0
        t, _ = ops.conv_lowrank_down(x.to(gpu_device), down.to(gpu_device), *_args(geo))
        assert np.array_equal(bits(t), bits(want)), f"census {fmt} {name} pixel {pixel}: {where(bits(t), bits(want))}"


# ---- conv_lowrank_grad ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.GRAD_GEOMETRIES))
@pytest.mark.parametrize("fmt", FMTS)
def test_conv_lowrank_grad_exact_sums(fmt, name, gpu_device):
    geo = C.GRAD_GEOMETRIES[name]
    m, k = C.sizes(geo)
    for rank in C.GRAD_RANKS[name]:
        x, g, acc, share = C.grad_case(name, rank, fmt)
        print(name, rank, fmt, "sensitivity", share)
        assert share >= SENSITIVITY_FLOOR
        xg, gg = x.to(gpu_device), g.to(gpu_device)
        slabs = -(-m // C.CLG_SLAB)
        assert ops.conv_lowrank_grad_workspace_bytes(x.shape, *_args(geo), rank) == (0 if slabs == 1 else slabs * k * rank * 4)
        for tag in C.OUT_TAGS:
            got = ops.conv_lowrank_grad(xg, gg, *_args(geo), C.grad_scale(tag), out_dtype=DT[tag])
            assert got.shape == (rank, k) and got.dtype == DT[tag]
            _same(_f32(got), C.grad_expected(acc, tag), "conv_lowrank_grad", fmt, name, rank, tag)


@pytest.mark.parametrize("fmt", FMTS)
def test_conv_lowrank_grad_twice_and_in_a_graph(fmt, gpu_device):
    """Three slabs: two calls give the same bits; a captured call, workspace included, replays the eager bits."""
    name, rank = "g9_3x3_three_slabs", 64
    geo = C.GRAD_GEOMETRIES[name]
    x, g, acc, _ = C.grad_case(name, rank, fmt)
    xg, gg = x.to(gpu_device), g.to(gpu_device)
    first = ops.conv_lowrank_grad(xg, gg, *_args(geo), 0.3, out_dtype=torch.bfloat16)
    _same(_f32(first), C.grad_expected(acc, "bf16", 0.3), "conv_lowrank_grad", fmt, "three slabs")
    again = ops.conv_lowrank_grad(xg, gg, *_args(geo), 0.3, out_dtype=torch.bfloat16)
    assert np.array_equal(bits(first), bits(again)), "two calls differ"
    nbytes = ops.conv_lowrank_grad_workspace_bytes(x.shape, *_args(geo), rank)
    assert nbytes == 3 * C.sizes(geo)[1] * rank * 4
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=gpu_device)
    eager = ops.conv_lowrank_grad(xg, gg, *_args(geo), 0.3, out_dtype=torch.bfloat16, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.conv_lowrank_grad(xg, gg, *_args(geo), 0.3, out_dtype=torch.bfloat16, workspace=ws)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(captured), bits(eager)) and np.array_equal(bits(eager), bits(first)), "graph replay differs"


@pytest.mark.parametrize("name", ("g1_3x3_ragged", "g2_3x3_stride2", "g5_conv1d_k5", "g7_3x2_mixed", "g9_3x3_three_slabs"))
@pytest.mark.parametrize("fmt", FMTS)
def test_conv_lowrank_grad_row_census(fmt, name, gpu_device):
    geo = C.GRAD_GEOMETRIES[name]
    m, _ = C.sizes(geo)
    for row in sorted({0, 63 % m, m // 2, C.CLG_SLAB % m, m - 1}):
        x, g, prod = C.grad_census(name, row, 24, fmt)
        got = ops.conv_lowrank_grad(x.to(gpu_device), g.to(gpu_device), *_args(geo), 1.0, out_dtype=torch.float32)
        assert np.array_equal(bits(got), bits(torch.from_numpy(prod))), f"census {fmt} {name} row {row}: {where(bits(got), bits(torch.from_numpy(prod)))}"
