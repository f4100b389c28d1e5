"""The direct form of the one-launch w8a8 Linear's 32 x 256 tile (csrc/gemm_aq.hip, DIRECT): no LDS ring for the weights -- every wave
loads the fragments of its own 32 weight rows from the fragment-ordered slab copy of the weight (sdnq_hip_aq_slab_pack) straight into the
registers its MFMAs read, three stages deep, and reloads each register with stage j + 3 behind the MFMA that read it.  All cases force
geometry 1 (tests/aq_internal.py), hand every one-launch call the slab copy, and pick the form through the library's hook
sdnq_internal_aq_direct: 0 = the ring form (the copy is ignored), anything else = the direct form.

Expected values never come from the form under test: they are the two-launch route's (sdnq_hip_rowquant + sdnq_hip_scaled_mm), the
ring slab form's, or -- in the placement census -- the weight array itself.  Equality of bits, no tolerance.

Placement census (as tests/test_gemm_aq_regslab.py): row m of x is one-hot (1.0 at column m mod K), weight scales 1, no bias, so
out[m][n] = W[n][m mod K] exactly and every output element names ONE weight byte: a wave that reads another block of the copy, a stage
in another register set, a refill that lands in the wrong sub-step's registers, a copy with two pieces swapped shows as a wrong element
and cannot cancel.

Shapes: K = 128 (one stage: fewer than the three register stages), 384 (exactly three), 640 (all five stages of the NJ = 5
instantiation: two refills), 768 (NJ = 10 with stages past K issued as filler), 1280 (all ten: every register set refilled twice or
more); N = 256 (one full tile), 512, 264 (a second tile of 8 columns: seven waves lie past N and read the tile's only block), 40 (n_lim
no multiple of 32: the second block holds 8 live rows and 24 copies of the last one); M = 32, 33, 64, 70 (full and ragged row blocks,
one and more than one of them)."""
import ctypes

import numpy as np
import pytest
import torch

from sdnq_amd import _lib
from tests import aq_internal as A

pytestmark = pytest.mark.gpu

from sdnq_amd import ops  # noqa: E402

RING = 0
DIRECT_STAGES = [1]  # form codes of the hook that run the direct form (one depth is built)
KS = [128, 384, 640, 768, 1280]  # 128 .. 640: the NJ = 5 instantiation; 768, 1280: NJ = 10
NS = [256, 512, 264, 40]
MS = [32, 33, 64, 70]
DTYPES = [torch.bfloat16, torch.float16]


def set_direct(stages: int) -> None:
    """-1: the library's default; 0: the ring form; anything else: the direct form (where the call passes the slab copy)."""
    _lib.load()
    f = getattr(ctypes.CDLL(_lib.LIB_PATH), "_Z23sdnq_internal_aq_directi")
    f.argtypes, f.restype = [ctypes.c_int], None
    f(stages)


@pytest.fixture(autouse=True)
def geometry_1():
    A.set_geometry(A.GEO_32x256)
    yield
    A.set_geometry(-1)
    set_direct(-1)


def _bits(t):
    return t.view(torch.int16)


def _hash_weight(n, k):
    """W[n][k] in [-127, 127]: a fixed integer hash of (n, k)."""
    with np.errstate(over="ignore"):
        nn = np.arange(n, dtype=np.uint32)[:, None]
        kk = np.arange(k, dtype=np.uint32)[None, :]
        h = nn * np.uint32(0x9E3779B1) ^ (kk * np.uint32(0x85EBCA77) + np.uint32(0x165667B1))
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(12)
    return ((h % np.uint32(255)).astype(np.int16) - 127).astype(np.int8)


def _random(m, n, k, seed, dev):
    """Full-entropy operands in float32 (cast per case): normal rows under log-normal row magnitudes, int8 weights over the whole range."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * torch.exp(torch.randn(m, 1, generator=g))
    b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g)
    sb = torch.rand(n, generator=g) * 0.02 + 1e-4
    bias = torch.randn(n, generator=g)
    return x.to(dev), b.to(dev), sb.to(dev), bias.to(dev)


def _fused(stages, x, b, sb, bias, dtype, slab=None):
    set_direct(stages)
    return ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, dtype, ops.aq_slab_pack(b) if slab is None else slab)


def _assert_all_forms(x, b, sb, bias, dtype, what):
    """Every direct form == the ring slab form == the two-launch route, bit for bit."""
    y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, dtype)
    slab = ops.aq_slab_pack(b)
    ring = _fused(RING, x, b, sb, bias, dtype, slab)
    got = [_fused(r, x, b, sb, bias, dtype, slab) for r in DIRECT_STAGES]
    torch.cuda.synchronize()
    assert torch.equal(_bits(ring), _bits(y2)), ("ring form vs two launches", what, int((_bits(ring) != _bits(y2)).sum()))
    for r, y in zip(DIRECT_STAGES, got):
        assert torch.equal(_bits(y), _bits(y2)), ("direct form vs two launches", r, what, int((_bits(y) != _bits(y2)).sum()))
        assert torch.equal(_bits(y), _bits(ring)), ("direct form vs ring form", r, what, int((_bits(y) != _bits(ring)).sum()))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_placement_census(k, n, gpu_device):
    m = k
    w_np = _hash_weight(n, k)
    b = torch.from_numpy(w_np).to(gpu_device)
    sb = torch.ones(n, dtype=torch.float32, device=gpu_device)
    slab = ops.aq_slab_pack(b)
    for dtype in DTYPES:
        expected = torch.from_numpy(w_np.T.astype(np.float32).copy()).to(dtype)  # out[m][n] = W[n][m mod K], M = K
        x = torch.zeros(m, k, dtype=dtype)
        x[torch.arange(m), torch.arange(m) % k] = 1.0
        x = x.to(gpu_device)
        y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, None, dtype)
        got = [_fused(r, x, b, sb, None, dtype, slab) for r in DIRECT_STAGES]
        torch.cuda.synchronize()
        assert torch.equal(_bits(y2.cpu()), _bits(expected)), "the census array is not what the two-launch route computes"
        for r, y in zip(DIRECT_STAGES, got):
            bad = (_bits(y.cpu()) != _bits(expected)).nonzero()
            assert bad.numel() == 0, (r, k, n, dtype, bad.shape[0], bad[:8].tolist())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_random_operands_every_row_count_dtype_and_bias(k, n, gpu_device):
    xf, b, sb, biasf = _random(max(MS), n, k, 131 * n + k, gpu_device)
    for dtype in DTYPES:
        for m in MS:
            x = xf[:m].to(dtype)
            for bias in (None, biasf.to(dtype), biasf):  # no bias, a bias of the activation dtype, a float32 bias
                _assert_all_forms(x, b, sb, bias, dtype, (m, n, k, dtype, None if bias is None else bias.dtype))


@pytest.mark.parametrize("k", [640, 1280])  # one per NJ
def test_strided_activation_rows(k, gpu_device):
    m, n = 70, 512
    xf, b, sb, biasf = _random(m, n, k, k + 5, gpu_device)
    for dtype in DTYPES:
        wide = torch.full((m, k + 136), 3.0e4, dtype=dtype, device=gpu_device)  # (a read past K would raise the row's amax)
        wide[:, :k] = xf.to(dtype)
        bias = biasf.to(dtype)
        ref, _, _ = ops.linear_w8a8(ops.MM_I8, xf.to(dtype), b, sb, bias, dtype)
        for r in DIRECT_STAGES:
            y = _fused(r, wide[:, :k], b, sb, bias, dtype)
            torch.cuda.synchronize()
            assert torch.equal(_bits(y), _bits(ref)), (r, k, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(64, 512, 1280), (70, 264, 768), (33, 40, 640)])
def test_nan_zero_and_inf_rows(shape, dtype, gpu_device):
    m, n, k = shape
    xf, b, sb, biasf = _random(m, n, k, 11 * m + n + k, gpu_device)
    x = xf.to(dtype)
    # a nan row, an all-zero row and two inf rows: the second amax sweep and the quantizer's general path, in waves that also hold plain rows
    x[5, 3] = float("nan")
    x[m - 2] = 0
    x[m // 2, k - 1] = float("-inf")
    x[9, k // 2] = float("inf")
    _assert_all_forms(x, b, sb, biasf.to(dtype), dtype, (shape, dtype))


def test_any_hook_value_with_or_without_the_copy(gpu_device):
    """Whatever the hook is given, and with or without the slab copy, a built kernel runs and the bits are the two-launch route's."""
    m, n, k = 33, 256, 1280
    xf, b, sb, biasf = _random(m, n, k, 77, gpu_device)
    x, bias = xf.to(torch.bfloat16), biasf.to(torch.bfloat16)
    ref, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, torch.bfloat16)
    for stages in (-1, 1, 2, 5, 7, 9, 16, 17, 21, 25, 35, 36, 1000):
        y = _fused(stages, x, b, sb, bias, torch.bfloat16)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(ref)), stages
    for stages in (-1, 0, 1, 3):
        set_direct(stages)
        y = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, torch.bfloat16)  # no slab copy: sdnq_hip_linear_w8a8_fused
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(ref)), stages
