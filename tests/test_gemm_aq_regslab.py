"""The wave-private slab form of the one-launch w8a8 Linear (csrc/gemm_aq.hip, the 32 x 256 tile): every wave moves its own 32 weight
rows, drains each landed K stage from its ring slot into registers on its own counted wait -- the first two stages while the rows are
quantized, the others in a K loop without a barrier -- and refills the slot at once.  All cases force geometry 1 through the library's
hook (tests/aq_internal.py).

Expected values never come from the one-launch route: they are the two-launch route's (sdnq_hip_rowquant + sdnq_hip_scaled_mm), the CPU
oracle's, or -- in the placement census -- the weight array itself.  Equality of bits, no tolerance.

Placement census: row m of x is one-hot (1.0 at column m mod K), so its scale is fl(1 / 127) and its only code 127; with weight scales
of 1 and no bias, out[m][n] = cast(f32(127 W[n][k]) * fl(1 / 127)) = W[n][k] exactly (|W| <= 127 has 7 significant bits; the product is
off by one part in 10^7 and the 16-bit cast rounds it back).  Every output element names one weight byte: a piece that lands in another
wave's rows, a stage in another register or ring slot shows as a wrong element, and M = K rows hit every k.

Shapes, the smallest at which each branch of the form can fail: K = 128 (one stage, fewer than the ring's three slots and than the two
stages drained under the quantization), 384 (exactly the ring), 512 (the first refilled slot read), 640 (all five stages of the NJ = 5
instantiation), 768 (the NJ = 10 instantiation, stages past K issued as filler), 1280 (all ten); N = 256 (one full tile), 264 (one column block of a second tile holds 8 columns, seven waves' blocks
lie past N), 40 (most waves past N in the only tile), 512; M = 33, 32, 1, 70 (ragged and single row blocks)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import aq_internal as A
from tests.modules_util import to_f32_numpy

pytestmark = pytest.mark.gpu

from sdnq_amd import ops  # noqa: E402

KS = [128, 384, 512, 640, 768, 1280]
NS = [256, 264, 40, 512]
MS = [33, 32, 1, 70]
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def geometry_1():
    A.set_geometry(A.GEO_32x256)
    yield
    A.set_geometry(-1)


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


def _random(m, n, k, dtype, seed, dev, bias_dtype=None):
    """Full-entropy operands: normal rows under log-normal row magnitudes, int8 weights over the whole range."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(m, k, generator=g) * torch.exp(torch.randn(m, 1, generator=g))).to(dtype)
    b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g)
    sb = torch.rand(n, generator=g) * 0.02 + 1e-4
    bias = torch.randn(n, generator=g).to(bias_dtype or dtype)
    return x.to(dev), b.to(dev), sb.to(dev), bias.to(dev)


def _oracle_int8(x, b, sb, bias, dtype, rows=None):
    xf = x.float().cpu().numpy()
    if rows is not None:
        xf = xf[rows]
    with np.errstate(all="ignore"):
        xq_o, xs_o, _ = O.rowquant(xf, "int8")
    return O.scaled_mm("int8", xq_o, b.cpu().numpy(), xs_o.reshape(-1), sb.cpu().numpy(), None if bias is None else bias.float().cpu().numpy(),
                       "bf16" if dtype == torch.bfloat16 else "f16")


def test_hash_weight_distinguishes_neighbouring_rows_stages_and_pieces():
    w = _hash_weight(512, 1280).astype(np.int32)
    assert w.min() == -127 and w.max() == 127
    # rows 8 apart (pieces), 32 apart (waves), columns 16 / 128 apart (chunks, stages): the arrays differ almost everywhere
    for dn, dk in ((8, 0), (32, 0), (0, 16), (0, 128), (0, 384), (1, 0)):
        a, c = w[dn:, dk:], w[: w.shape[0] - dn, : w.shape[1] - dk]
        assert (a != c).mean() > 0.98, (dn, dk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_placement_census(k, n, dtype, gpu_device):
    m = k
    w_np = _hash_weight(n, k)
    expected = torch.from_numpy(w_np.T.astype(np.float32).copy()).to(dtype)  # out[m][n] = W[n][m mod K], M = K
    x = torch.zeros(m, k, dtype=dtype)
    x[torch.arange(m), torch.arange(m) % k] = 1.0
    x, b = x.to(gpu_device), torch.from_numpy(w_np).to(gpu_device)
    sb = torch.ones(n, dtype=torch.float32, device=gpu_device)
    y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, None, dtype)
    y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, None, dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y2.cpu()), _bits(expected)), "the census array is not what the two-launch route computes"
    bad = (_bits(y1.cpu()) != _bits(expected)).nonzero()
    assert bad.numel() == 0, (k, n, dtype, bad.shape[0], bad[:8].tolist())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_random_operands_every_row_count_dtype_and_bias(k, n, gpu_device):
    for m in MS:
        for dtype in DTYPES:
            for bias_dtype in (None, dtype, torch.float32):
                x, b, sb, bias = _random(m, n, k, dtype, 131 * m + 7 * n + k, gpu_device, bias_dtype or dtype)
                bb = None if bias_dtype is None else bias
                y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bb, dtype)
                y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bb, dtype)
                torch.cuda.synchronize()
                assert torch.equal(_bits(y1), _bits(y2)), (m, n, k, dtype, bias_dtype, int((_bits(y1) != _bits(y2)).sum()))


@pytest.mark.parametrize("k", [640, 1280])  # one per NJ
def test_fp8_codes(k, gpu_device):
    m, n = 70, 264
    for dtype in DTYPES:
        x, _, sb, bias = _random(m, n, k, dtype, 3 * k + 1, gpu_device)
        g = torch.Generator().manual_seed(k)
        b = (torch.randn(n, k, generator=g) * 50).clamp(-448, 448).to(torch.float8_e4m3fn).to(gpu_device)
        for bb in (bias, None):
            y2, _, _ = ops.linear_w8a8(ops.MM_FP8, x, b, sb, bb, dtype)
            y1 = ops.linear_w8a8_fused(ops.MM_FP8, x, b, sb, bb, dtype)
            torch.cuda.synchronize()
            assert torch.equal(_bits(y1), _bits(y2)), (k, dtype, bb is not None, int((_bits(y1) != _bits(y2)).sum()))


@pytest.mark.parametrize("k", [640, 1280])
def test_strided_activation_rows(k, gpu_device):
    m, n = 70, 512
    x, b, sb, bias = _random(m, n, k, torch.bfloat16, k + 5, gpu_device)
    wide = torch.full((m, k + 136), 3.0e4, dtype=torch.bfloat16, device=gpu_device)  # (a read past K would raise the row's amax)
    wide[:, :k] = x
    ref, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, torch.bfloat16)
    y = ops.linear_w8a8_fused(ops.MM_I8, wide[:, :k], b, sb, bias, torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(64, 512, 1280), (70, 264, 768)])
def test_full_entropy_and_nan_zero_inf_rows(shape, dtype, gpu_device):
    m, n, k = shape
    x, b, sb, bias = _random(m, n, k, dtype, 11 * m + n + k, gpu_device)
    # plain rows first: the two-launch route and the oracle
    y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, dtype)
    y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y1), _bits(y2)), (shape, dtype, int((_bits(y1) != _bits(y2)).sum()))
    assert np.array_equal(to_f32_numpy(y1), _oracle_int8(x, b, sb, bias, dtype)), (shape, dtype)
    # a nan row, an all-zero row and an inf row: the second amax sweep and the quantizer's general path, in waves that also hold plain rows
    x[5, 3] = float("nan")
    x[m - 2] = 0
    x[34, k - 1] = float("-inf")
    x[9, k // 2] = float("inf")
    y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, dtype)
    y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y1), _bits(y2)), (shape, dtype, int((_bits(y1) != _bits(y2)).sum()))
    ordinary = torch.isfinite(x.float()).all(dim=1).cpu().numpy()
    assert np.array_equal(to_f32_numpy(y1)[ordinary], _oracle_int8(x, b, sb, bias, dtype, rows=ordinary)), (shape, dtype)
