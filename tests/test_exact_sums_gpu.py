"""Bit-exact GPU tests of the floating-point matrix-core GEMMs on exact-sum inputs (tests/exact_inputs.py).

On operands of small integers times one power of two per row, every product and every partial sum is an integer that float32 and
the MFMA's adder hold exactly (span measured in profiles/mfma_sum_probe.txt), so the result cannot depend on the tile schedule, the
LDS ring, the K split or the fragment layout -- and the CPU oracle's double accumulation is the bit-exact expected value.  One-hot
operands (one product per output, arbitrary values) need not even that premise.  Every output element of every case is compared
with np.array_equal: a K element dropped, duplicated or paired with the wrong partner in one row of one tail tile fails
(tests/test_exact_inputs.py shows that on the CPU model).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import exact_inputs as X
from tests.modules_util import to_f32_numpy

pytestmark = pytest.mark.gpu

from sdnq_amd import _lib, ops  # noqa: E402

TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


@pytest.fixture()
def tile_override():
    lib = _lib.load()
    yield lib.sdnq_hip_set_tile_override
    lib.sdnq_hip_set_tile_override(-1)


def _scales(m, n, seed):
    g = torch.Generator().manual_seed(seed)
    sa = torch.rand(m, generator=g) * 0.02 + 1e-4
    sb = torch.rand(n, generator=g) * 0.02 + 1e-4
    bias = torch.randn(n, generator=g).to(torch.bfloat16)
    return sa, sb, bias


class _Fp8Shape:
    """The operand sets of one ragged shape (dense exact-sum + one one-hot set per shift), resident on the GPU, with the oracle's
    answer per (set, bias, output dtype) computed once and shared by every tile configuration."""

    def __init__(self, shape, dev):
        m, n, k = self.shape = shape
        self.sa, self.sb, self.bias = _scales(m, n, m + 3 * n)
        sets = [("dense", X.exact_operands(m, n, k, seed=m + n + k, fmt="fp8"))]
        sets += [(f"one-hot shift {s}", X.one_hot_operands(m, n, k, s, "fp8")) for s in X.one_hot_shifts(k)]
        self.sets = [(name, ops_.codes(), ops_.a.to(dev), ops_.b.to(dev)) for name, ops_ in sets]
        self.dev = (self.sa.to(dev), self.sb.to(dev), self.bias.to(dev))
        self.refs = {}

    def ref(self, i, with_bias, tag):
        key = (i, with_bias, tag)
        if key not in self.refs:
            a, b = self.sets[i][1]
            self.refs[key] = O.scaled_mm("fp8", a, b, self.sa.numpy(), self.sb.numpy(), self.bias.float().numpy() if with_bias else None, tag)
        return self.refs[key]

    def check(self, tile, out_dtype):
        sa, sb, bias = self.dev
        for i, (name, _, a, b) in enumerate(self.sets):
            for with_bias in (True, False):
                out = ops.scaled_mm(ops.MM_FP8, a, b, sa, sb, bias if with_bias else None, out_dtype)
                got, ref = to_f32_numpy(out), self.ref(i, with_bias, TAG[out_dtype])
                assert np.array_equal(got, ref), (tile, self.shape, name, with_bias, TAG[out_dtype], _where(got, ref))


def _where(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} of {ref.size} differ, rows {bad[:, 0].min()}..{bad[:, 0].max()}, columns {bad[:, 1].min()}..{bad[:, 1].max()}, first {tuple(bad[0])}: " \
           f"got {got[tuple(bad[0])]!r} want {ref[tuple(bad[0])]!r}"


@functools.lru_cache(maxsize=None)
def _fp8_shape(shape, dev):
    return _Fp8Shape(shape, dev)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 17, 19, 20, 25, 28])
def test_fp8_every_tile_configuration_bit_exact_vs_oracle(tile, gpu_device, tile_override):
    """Every configuration of launch_tiles with the fp8 fragment path (two 16-byte chunks per lane, 64 bytes of K per MFMA), bf16
    output, M / N / K tails, K shorter than a stage.  (Id 28 falls through to the heuristics for fp8: compared all the same.)"""
    for shape in X.RAGGED_SHAPES:
        case = _fp8_shape(shape, gpu_device)
        tile_override(tile)
        case.check(tile, torch.bfloat16)


@pytest.mark.parametrize("tile", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("out_dtype", [torch.float16, torch.float32])
def test_fp8_f16_and_f32_outputs_bit_exact_vs_oracle(tile, out_dtype, gpu_device, tile_override):
    """float32 output keeps every bit of the accumulator: the configurations PP_OK leaves for it, and the heuristics."""
    for shape in X.RAGGED_SHAPES:
        case = _fp8_shape(shape, gpu_device)
        tile_override(tile)
        case.check(tile, out_dtype)


@pytest.mark.parametrize("shape", X.MODEL_SHAPES)
def test_fp8_model_size_default_heuristics_bit_exact(shape, gpu_device):
    """The schedules the heuristics pick at model size: first / last 64 rows and a middle slab against the oracle, the whole output
    against the int64 sums pushed through the float32 epilogue, three runs with identical bits."""
    m, n, k = shape
    ex = X.exact_operands(m, n, k, seed=n + k, fmt="fp8")
    assert ex.span_bits <= X.B["fp8"]
    sa, sb, bias = _scales(m, n, n)
    a, b = ex.a.to(gpu_device), ex.b.to(gpu_device)
    outs = [ops.scaled_mm(ops.MM_FP8, a, b, sa.to(gpu_device), sb.to(gpu_device), bias.to(gpu_device), torch.bfloat16) for _ in range(3)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))
    got = to_f32_numpy(outs[0])
    ac, bc = ex.codes()
    mid = (m // 2 - 37) if m > 256 else 64
    for rows in (slice(0, 64), slice(mid, mid + 64), slice(m - 64, m)):
        ref = O.scaled_mm("fp8", ac[rows], bc, sa.numpy()[rows], sb.numpy(), bias.float().numpy(), "bf16")
        assert np.array_equal(got[rows], ref), (shape, rows, _where(got[rows], ref))
    ints = X.expected_int(ex.ia, ex.ib)
    for r0 in range(0, m, 512):
        rows = slice(r0, min(m, r0 + 512))
        acc = ints[rows].astype(np.float64) * np.exp2((ex.ea[rows, None] + ex.eb[None, :]).astype(np.float64))
        want = X.epilogue(acc, sa.numpy()[rows], sb.numpy(), bias.float().numpy(), "bf16")
        assert np.array_equal(got[rows], want), (shape, rows, _where(got[rows], want))


# ---- every fp8 entry point that reaches the same template ------------------------------------------------------------------------
def _fp8_case(m, n, k, seed, dev, **kw):
    ex = X.exact_operands(m, n, k, seed=seed, fmt="fp8", **kw)
    sa, sb, bias = _scales(m, n, seed)
    return ex, sa, sb, bias, ex.a.to(dev), ex.b.to(dev)


@pytest.mark.parametrize("with_bias", [True, False])
def test_fp8_grouped_bit_exact_vs_oracle(with_bias, gpu_device):
    m, k, widths = 200, 640, [640, 1280, 640]
    ex, sa, _, _, a, _ = _fp8_case(m, sum(widths), k, 11, gpu_device)
    ac, bc = ex.codes()
    members, host, start = [], [], 0
    for i, n in enumerate(widths):
        _, sb, bias = _scales(m, n, 20 + i)
        members.append((ex.b[start:start + n].contiguous().to(gpu_device), sb.to(gpu_device), bias.to(gpu_device) if with_bias else None))
        host.append((bc[start:start + n], sb.numpy(), bias.float().numpy() if with_bias else None))
        start += n
    outs = ops.scaled_mm_grouped(ops.MM_FP8, a, sa.to(gpu_device), ops.GemmGroup(members), torch.bfloat16)
    for (bcn, sb, bias), out in zip(host, outs):
        ref = O.scaled_mm("fp8", ac, np.ascontiguousarray(bcn), sa.numpy(), sb, bias, "bf16")
        assert np.array_equal(to_f32_numpy(out), ref), _where(to_f32_numpy(out), ref)


def test_fp8_multi_bit_exact_vs_oracle(gpu_device):
    m, n, k, n_outs = 333, 1920, 528, 3
    ex, sa, sb, bias, a, b = _fp8_case(m, n, k, 12, gpu_device)
    ref = O.scaled_mm("fp8", *ex.codes(), sa.numpy(), sb.numpy(), bias.float().numpy(), "bf16")
    outs = ops.scaled_mm_multi(ops.MM_FP8, a, b, sa.to(gpu_device), sb.to(gpu_device), bias.to(gpu_device), torch.bfloat16, n_outs)
    for i, out in enumerate(outs):
        want = ref[:, i * (n // n_outs):(i + 1) * (n // n_outs)]
        assert np.array_equal(to_f32_numpy(out), want), (i, _where(to_f32_numpy(out), want))


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
def test_fp8_nchw_bit_exact_vs_oracle(out_dtype, gpu_device):
    batch, pixels, n, k = 3, 136, 392, 528   # m = 408: ragged against every tile height, images that start inside a tile
    m = batch * pixels
    ex, sa, sb, bias, a, b = _fp8_case(m, n, k, 13, gpu_device)
    ref = O.scaled_mm("fp8", *ex.codes(), sa.numpy(), sb.numpy(), bias.float().numpy(), TAG[out_dtype])
    out = ops.scaled_mm_nchw(ops.MM_FP8, a, b, sa.to(gpu_device), sb.to(gpu_device), bias.to(gpu_device), out_dtype, batch, pixels)
    got = to_f32_numpy(out.permute(0, 2, 1).reshape(m, n))
    assert np.array_equal(got, ref), _where(got, ref)


@pytest.mark.parametrize("m,n,k,lda", [(300, 392, 528, 1056), (257, 264, 48, 80), (100, 136, 16, 208), (129, 64, 112, 128)])
def test_fp8_strided_bit_exact_vs_oracle(m, n, k, lda, gpu_device):
    """Column slices of a wider activation (lda > K), K shorter than one 128-byte stage, output channels inside a wider row."""
    ex, sa, sb, bias, _, b = _fp8_case(m, n, k, 14, gpu_device)
    ref = O.scaled_mm("fp8", *ex.codes(), sa.numpy(), sb.numpy(), bias.float().numpy(), "bf16")
    col0 = 16
    wide = X._arbitrary(np.random.default_rng(0), (m, lda), "fp8")   # whatever lies beside the slice must not leak in
    wide[:, col0:col0 + k] = ex.a
    wide = wide.to(gpu_device)
    out = torch.full((m, n + 24), 7.0, dtype=torch.bfloat16, device=gpu_device)
    ops.scaled_mm_into(ops.MM_FP8, wide[:, col0:col0 + k], b, sa.to(gpu_device), sb.to(gpu_device), bias.to(gpu_device), out, 8)
    got = to_f32_numpy(out)
    assert np.array_equal(got[:, 8:8 + n], ref), _where(got[:, 8:8 + n], ref)
    assert (got[:, :8] == 7.0).all() and (got[:, 8 + n:] == 7.0).all()
    # the same slice through the entry point of the zero-point epilogues (no such term: an fp8 layer has none)
    out2 = torch.full((m, n + 24), 7.0, dtype=torch.bfloat16, device=gpu_device)
    ops.scaled_mm_zp_into(ops.MM_FP8, wide[:, col0:col0 + k], b, sa.to(gpu_device), sb.to(gpu_device), bias.to(gpu_device), None, None, None, None, 0, out2, 8)
    got2 = to_f32_numpy(out2)
    assert np.array_equal(got2[:, 8:8 + n], ref), _where(got2[:, 8:8 + n], ref)
    assert (got2[:, :8] == 7.0).all() and (got2[:, 8 + n:] == 7.0).all()


@pytest.mark.parametrize("m,n,k,r", [(300, 392, 528, 32), (1031, 264, 1296, 16)])
def test_fp8_lowrank_bit_exact_vs_oracle(m, n, k, r, gpu_device):
    """The low-rank (SVD) epilogue: t [M,R] and svd_up [N,R] take exact-sum bf16 values and the bias one that is an integer in the
    units of every low-rank sum, so the bf16 low-rank bias is exact before its one rounding; the main product is exact as above."""
    ex, sa, sb, _, a, b = _fp8_case(m, n, k, 15, gpu_device)
    lr = X.exact_operands(m, n, r, seed=16, fmt="bf16", density=1.0, e_window=(-6, -1))
    bias = X.exact_bias(lr, 17)
    t, up = lr.codes()
    bias2d = O.lowrank_bias(t, up, bias, "bf16")
    ref = O.scaled_mm("fp8", *ex.codes(), sa.numpy(), sb.numpy(), bias2d, "bf16")
    out = ops.scaled_mm_lowrank(ops.MM_FP8, a, b, sa.to(gpu_device), sb.to(gpu_device), torch.from_numpy(bias).to(torch.bfloat16).to(gpu_device),
                                lr.a.to(gpu_device), lr.b.to(gpu_device), None, None, torch.bfloat16)
    got = to_f32_numpy(out)
    assert np.array_equal(got, ref), _where(got, ref)


@pytest.mark.parametrize("m,n,k", [(300, 392, 528), (513, 1288, 208), (33, 72, 16)])
def test_fp8_bf16_scale_chain_bit_exact_vs_oracle(m, n, k, gpu_device):
    """sdnq_hip_scaled_mm_lp: accumulator, activation-scale product and result each rounded to bf16.  Power-of-two scales make the
    two multiplications exact, so only the accumulator's rounding (of an exact float32) and the bias fma round."""
    ex, _, _, bias, a, b = _fp8_case(m, n, k, 18, gpu_device)
    rng = np.random.default_rng(19)
    sa = np.exp2(rng.integers(-9, -3, size=m)).astype(np.float32)
    sb = np.exp2(rng.integers(-9, -3, size=n)).astype(np.float32)
    for bs in (bias, None):
        ref = O.scaled_mm_lp("fp8", *ex.codes(), sa, sb, None if bs is None else bs.float().numpy(), "bf16")
        out = ops.scaled_mm_lp(ops.MM_FP8, a, b, torch.from_numpy(sa).to(gpu_device), torch.from_numpy(sb).to(gpu_device),
                               None if bs is None else bs.to(gpu_device))
        got = to_f32_numpy(out)
        assert np.array_equal(got, ref), (bs is None, _where(got, ref))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(64, 128, 128), (333, 1288, 1152), (1000, 640, 640), (257, 264, 1280)])
def test_fp8_one_launch_linear_bit_exact_vs_oracle(shape, dtype, gpu_device):
    """linear_w8a8_fused(MM_FP8): the GEMM quantizes its own rows.  Each activation row is an exact-sum e4m3 row with one element of
    448 planted in it, times a power of two: amax / 448 is that power of two, so the row quantizer reproduces the codes exactly
    (checked against the oracle's rowquant and the two-launch route's codes) and the sums stay exact."""
    m, n, k = shape
    ex = X.exact_operands(m, n, k, seed=m + k, fmt="fp8", e_window=(0, 6))
    ia = ex.ia.copy()
    cols = (np.arange(m) * 5 + 1) % k
    ia[np.arange(m), cols] = 7 * 2 ** (6 - ex.ea)   # 448 in units of 2^ea
    assert X.span_bits_of(ia, ex.ib) <= X.B["fp8"]
    codes = X.to_format(ia, ex.ea, "fp8")
    assert np.array_equal(codes.float().numpy().astype(np.float64), ia * np.exp2(ex.ea.astype(np.float64))[:, None])
    j = np.random.default_rng(m).integers(-3, 4, size=m)
    x = (codes.float() * torch.from_numpy(np.exp2(j.astype(np.float32)))[:, None]).to(dtype)
    assert torch.equal(x.float(), codes.float() * torch.from_numpy(np.exp2(j.astype(np.float32)))[:, None])
    xq_o, xs_o, _ = O.rowquant(x.float().numpy(), "fp8")
    assert np.array_equal(xq_o, codes.view(torch.uint8).numpy()) and np.array_equal(xs_o, np.exp2(j.astype(np.float32)))
    _, sb, bias = _scales(m, n, n)
    bias = bias.to(dtype)
    xd, bd = x.to(gpu_device), ex.b.to(gpu_device)
    for bs in (bias, None):
        ref = O.scaled_mm("fp8", xq_o, ex.codes()[1], xs_o, sb.numpy(), None if bs is None else bs.float().numpy(), TAG[dtype])
        y2, xq, xs = ops.linear_w8a8(ops.MM_FP8, xd, bd, sb.to(gpu_device), None if bs is None else bs.to(gpu_device), dtype)
        assert np.array_equal(xq.view(torch.uint8).cpu().numpy(), xq_o) and np.array_equal(xs.cpu().numpy().reshape(-1), xs_o)
        y1 = ops.linear_w8a8_fused(ops.MM_FP8, xd, bd, sb.to(gpu_device), None if bs is None else bs.to(gpu_device), dtype)
        for name, y in (("one launch", y1), ("two launches", y2)):
            got = to_f32_numpy(y)
            assert np.array_equal(got, ref), (name, shape, dtype, bs is None, _where(got, ref))


# ---- the 16-bit float paths ------------------------------------------------------------------------------------------------------
FLOAT_TILES = (-1, 0, 1, 2, 3, 4)
FLOAT_SHAPES = X.W8A16_SHAPES + ((300, 392, 512), (257, 264, 128), X.FLOAT_EXTRA_SHAPES[0])
W8_SHAPES = FLOAT_SHAPES[:-1] + (X.FLOAT_EXTRA_SHAPES[1],)   # sdnq_hip_linear_w8a16 takes K % 16 == 0


@functools.lru_cache(maxsize=None)
def _float_case(shape, fmt):
    m, n, k = shape
    ex = X.exact_operands(m, n, k, seed=m + 2 * n, fmt=fmt)
    bias = X.exact_bias(ex, 5)
    xa, wb = ex.codes()
    return ex, bias, {True: O.linear_float(xa, wb, bias, fmt), False: O.linear_float(xa, wb, None, fmt)}


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_float_gemm_bit_exact_vs_oracle(dt, gpu_device, tile_override):
    """sdnq_hip_linear_float (every use_quantized_matmul=False layer after its dequantize) on forced tiles and ragged shapes."""
    for shape in FLOAT_SHAPES:
        ex, bias, refs = _float_case(shape, TAG[dt])
        x, w, bd = ex.a.to(gpu_device), ex.b.to(gpu_device), torch.from_numpy(bias).to(dt).to(gpu_device)
        for tile in FLOAT_TILES:
            tile_override(tile)
            for with_bias in (True, False):
                got = to_f32_numpy(ops.linear_float(x, w, bd if with_bias else None))
                assert np.array_equal(got, refs[with_bias]), (shape, TAG[dt], tile, with_bias, _where(got, refs[with_bias]))


@pytest.mark.parametrize("wdt", ["int8", "uint8"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_fused_dequant_gemm_bit_exact_vs_oracle(wdt, dt, gpu_device, tile_override):
    """sdnq_hip_linear_w8a16: int8 codes in [-4, 4] (uint8: 0..8 with a zero point of -4 scale) and power-of-two row scales, so the
    in-register dequantize gives exactly the exact-sum weights and the float-linear oracle on those weights is the expected value."""
    for shape in W8_SHAPES:
        ex, bias, refs = _float_case(shape, TAG[dt])
        scale = np.exp2(ex.eb.astype(np.float32))
        if wdt == "int8":
            w, zp = torch.from_numpy(ex.ib.astype(np.int8)), None
        else:
            w, zp = torch.from_numpy((ex.ib + 4).astype(np.uint8)), torch.from_numpy(-4 * scale).to(gpu_device)
        x, w, sc, bd = ex.a.to(gpu_device), w.to(gpu_device), torch.from_numpy(scale).to(gpu_device), torch.from_numpy(bias).to(dt).to(gpu_device)
        for tile in FLOAT_TILES:
            tile_override(tile)
            for with_bias in (True, False):
                got = to_f32_numpy(ops.linear_w8a16(x, w, sc, zp, bd if with_bias else None))
                assert np.array_equal(got, refs[with_bias]), (shape, wdt, TAG[dt], tile, with_bias, _where(got, refs[with_bias]))


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_float16_scaled_mm_bit_exact(out_dtype, gpu_device, tile_override):
    """sdnq_hip_scaled_mm_f16 against the scaled oracle's epilogue on the exact float16 sums (and, with unit scales, against the
    float-linear oracle itself)."""
    for shape in FLOAT_SHAPES + (X.FLOAT_EXTRA_SHAPES[2],):
        m, n, k = shape
        ex = X.exact_operands(m, n, k, seed=m + 2 * n, fmt="f16")
        sa, sb, bias = _scales(m, n, k)
        acc = ex.acc()
        a, b = ex.a.to(gpu_device), ex.b.to(gpu_device)
        for tile in FLOAT_TILES:
            tile_override(tile)
            for bs in (bias, None):
                want = X.epilogue(acc, sa.numpy(), sb.numpy(), None if bs is None else bs.float().numpy(), TAG[out_dtype])
                got = to_f32_numpy(ops.scaled_mm_f16(a, b, sa.to(gpu_device), sb.to(gpu_device), None if bs is None else bs.to(gpu_device), out_dtype))
                assert np.array_equal(got, want), (shape, TAG[out_dtype], tile, bs is None, _where(got, want))
        if out_dtype == torch.float16:
            one_m, one_n = torch.ones(m, device=gpu_device), torch.ones(n, device=gpu_device)
            got = to_f32_numpy(ops.scaled_mm_f16(a, b, one_m, one_n, None, out_dtype))
            ref = O.linear_float(*ex.codes(), None, "f16")
            assert np.array_equal(got, ref), (shape, "unit scales", _where(got, ref))
