"""Bit-exact tests of sdnq_hip_merge_lowrank on the GPU.  The planted weights and factors of tests/dora_util.py make
e = w + SCALE * up @ down exact in float32 in any summation order, so the merged codes, scales and zero points must be torch.equal to
ops.quantize_weight applied to the float32 matrix e -- and e is built HERE, on the host, from the planted integers, not by the kernel
under test; that it is exact is asserted (D.normsq_expected's checks of the rank sum and of the fma, and a float32 round trip of e) before
anything is compared, so a case whose e is inexact fails instead of passing by luck.

Shapes: N = 24 (a full 16-row block and a ragged one); K = 272 and 528 (one and two full 256-column chunks plus a 16-column tail),
rounded up to a multiple of the group size where the group does not divide them (the tail is then one group); rank 8 and 40 (a ragged
second 32-rank step)."""
import dataclasses

import numpy as np
import pytest
import torch

from sdnq_amd import ops
from tests import dora_util as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every non-codebook bucket of the dequantizer, and the two integer formats of the flagship workloads at the groups that cross waves
# through LDS (128, 256) and row-wise (two sweeps)
FORMATS = tuple(f for f in D.FORMATS if not f.codebook) + (D.Fmt("int8", 128), D.Fmt("int8", 256), D.Fmt("uint4", 128), D.Fmt("uint4", 256),
                                                           D.Fmt("uint4"))
SHAPES = ((24, 272, 8), (24, 528, 40))


def _k(fmt: D.Fmt, k: int) -> int:
    return k if not fmt.group else -(-k // fmt.group) * fmt.group


def _t(a: np.ndarray, tag: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(D.DT[tag]).to(DEV)


def _exact_e(wt: D.Weight, up, down, row_scale=None) -> torch.Tensor:
    """e [n, k] float32 on the device, from the float64 restatement, with its exactness asserted."""
    if up is not None:
        D.normsq_expected(wt.w, up, down, D.SCALE, wt.er)  # asserts: the rank sum and the fma are exact in float32 in every order
    _, e = D.normsq_f64(wt.w, up, down, D.SCALE)
    if row_scale is not None:
        e = row_scale.astype(np.float64)[:, None] * e
    e32 = e.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), e), "the expected matrix is not exact in float32"
    return torch.from_numpy(e32).to(DEV)


def _check(got, e: torch.Tensor, fmt: D.Fmt, what: str) -> None:
    want = ops.quantize_weight(e, fmt.wdt, fmt.group or e.shape[1])
    for g, w, name in zip(got, want, ("codes", "scale", "zero point")):
        assert (g is None) == (w is None), f"{what}: {name}"
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype} {tuple(g.shape)}, the quantizer's {w.dtype} {tuple(w.shape)}"
        g8, w8 = g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)  # bits, not values: NaN and -0.0 count
        bad = int((g8 != w8).sum())
        assert bad == 0, f"{what}: {bad} of {g8.numel()} bytes of the {name} differ from quantize_weight(e)"


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: f.id)
def test_merged_codes_are_the_quantizers_on_exact_operands(fmt):
    for i, (n, k, rank) in enumerate(SHAPES):
        k = _k(fmt, k)
        wt = D.plant_weight(fmt, n, k, seed=500 + i)
        qw = wt.device(DEV)
        up, down = D.plant_factors(n, k, rank, wt.er, seed=600 + i)
        e = _exact_e(wt, up, down)
        for tag in ("bf16", "f16"):
            got = ops.merge_lowrank(qw, _t(up, tag), _t(down, tag), D.SCALE, weights_dtype=fmt.wdt)
            _check(got, e, fmt, f"{fmt.id} {n}x{k} rank {rank} {tag}")
        again = ops.merge_lowrank(qw, _t(up, "bf16"), _t(down, "bf16"), D.SCALE)  # the format found from the descriptor; the same bits
        _check(again, e, fmt, f"{fmt.id} {n}x{k} rank {rank}: a second call")


def _rows(wt: D.Weight, r0: int, r1: int) -> D.Weight:
    cut = lambda a: None if a is None else np.ascontiguousarray(a[r0:r1])  # noqa: E731
    return dataclasses.replace(wt, n=r1 - r0, stored=np.ascontiguousarray(wt.stored.reshape(wt.n, -1)[r0:r1]).reshape(-1), scale=cut(wt.scale),
                               zp=cut(wt.zp), w=cut(wt.w), er=cut(wt.er))


@pytest.mark.parametrize("fmt", (D.Fmt("int8"), D.Fmt("uint4", 64), D.Fmt("int8", 128)), ids=lambda f: f.id)
def test_rows_do_not_depend_on_their_block(fmt):
    n, k, rank = 40, _k(fmt, 528), 40
    wt = D.plant_weight(fmt, n, k, seed=700)
    up, down = D.plant_factors(n, k, rank, wt.er, seed=701)
    full = ops.merge_lowrank(wt.device(DEV), _t(up, "bf16"), _t(down, "bf16"), D.SCALE, weights_dtype=fmt.wdt)
    _check(full, _exact_e(wt, up, down), fmt, f"{fmt.id} {n}x{k}: three blocks")
    alone = ops.merge_lowrank(_rows(wt, 16, 40).device(DEV), _t(up[16:40], "bf16"), _t(down, "bf16"), D.SCALE, weights_dtype=fmt.wdt)
    for f, a, name in zip(full, alone, ("codes", "scale", "zero point")):
        if f is not None:
            assert torch.equal(f.reshape(n, -1)[16:40], a.reshape(24, -1)), f"{fmt.id}: the {name} of rows 16 .. 39 depend on their block"


@pytest.mark.parametrize("fmt", (D.Fmt("int8"), D.Fmt("uint4", 64), D.Fmt("int5", 16), D.Fmt("uint4", 256), D.Fmt("float8_e4m3fn")),
                         ids=lambda f: f.id)
def test_row_scale_with_and_without_factors(fmt):
    n, k, rank = 24, _k(fmt, 272), 8
    wt = D.plant_weight(fmt, n, k, seed=800)
    qw = wt.device(DEV)
    up, down = D.plant_factors(n, k, rank, wt.er, seed=801)
    c = np.exp2(np.random.default_rng(802).integers(-2, 3, size=n)).astype(np.float32)  # powers of two: the multiply is exact
    cd = torch.from_numpy(c).to(DEV)
    got = ops.merge_lowrank(qw, _t(up, "f16"), _t(down, "f16"), D.SCALE, cd, weights_dtype=fmt.wdt)
    _check(got, _exact_e(wt, up, down, c), fmt, f"{fmt.id}: row scale on the merged weight")
    got = ops.merge_lowrank(qw, None, None, 1.0, cd, weights_dtype=fmt.wdt)
    _check(got, _exact_e(wt, None, None, c), fmt, f"{fmt.id}: the pure row rescale")


@pytest.mark.parametrize("fmt", (D.Fmt("int8"), D.Fmt("int8", 128), D.Fmt("uint4", 64), D.Fmt("uint4")), ids=lambda f: f.id)
def test_a_group_whose_delta_cancels_the_weight_takes_the_nan_path(fmt):
    """Row 5's first group: up[5] is one entry -2 * 2^er at rank 3 and down[3] the group's planted integers, so SCALE * acc == -w there and
    every e of the group is +0.0: scale 0, 0 / 0 = NaN, code 0 (unsigned: (e - zp) / s with zp = 0)."""
    n, k, rank, row, r0 = 24, _k(fmt, 272), 8, 5, 3
    group = fmt.group or k
    wt = D.plant_weight(fmt, n, k, seed=900)
    up, down = D.plant_factors(n, k, rank, wt.er, seed=901)
    unit = np.exp2(float(wt.er[row]))
    up[row] = 0.0
    up[row, r0] = -2.0 * unit
    down[:, :group] = 0.0
    down[r0, :group] = wt.w[row, :group] / unit
    e = _exact_e(wt, up, down)
    assert not bool(e[row, :group].any()) and bool(e[row - 1, :group].any())
    got = ops.merge_lowrank(wt.device(DEV), _t(up, "bf16"), _t(down, "bf16"), D.SCALE, weights_dtype=fmt.wdt)
    _check(got, e, fmt, f"{fmt.id}: a cancelled group")
    assert float(got[1].reshape(n, -1)[row, 0]) == 0.0


@pytest.mark.parametrize("group", (0, 128), ids=("row-wise", "group 128"))
def test_an_all_zero_group(group):
    """int8 codes are plain bytes: row 9's first group is stored as zeros and its row of up is zero -- w == 0 and delta == 0 there."""
    fmt = D.Fmt("int8", group)
    n, k, rank, row = 24, _k(fmt, 272), 8, 9
    g = group or k
    wt = D.plant_weight(fmt, n, k, seed=950)
    wt.stored.reshape(n, k)[row, :g] = 0
    wt.w[row, :g] = 0.0
    up, down = D.plant_factors(n, k, rank, wt.er, seed=951)
    up[row] = 0.0
    e = _exact_e(wt, up, down)
    assert not bool(e[row, :g].any())
    got = ops.merge_lowrank(wt.device(DEV), _t(up, "bf16"), _t(down, "bf16"), D.SCALE, weights_dtype=fmt.wdt)
    _check(got, e, fmt, f"{fmt.id}: an all-zero group")
    assert not bool(got[0].reshape(n, k)[row, :g].any())
