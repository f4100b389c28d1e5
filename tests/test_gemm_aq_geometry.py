"""GPU parity of the one-launch w8a8 Linear on EACH tile geometry of csrc/gemm_aq.hip, forced through the library's internal hook
(tests/aq_internal.py): 64 x 128 with 4 ring slots and 32 x 256 with 3.

The cases of tests/test_gemm_aq.py, on both geometries whatever the shape rule would pick: the same bits as the two-launch route
(sdnq_hip_rowquant + sdnq_hip_scaled_mm) and, for int8, as the CPU oracle -- equality, no tolerance.  Added here: M not a multiple of
32, N edges inside a 256-wide tile, K of 1, 5 and 10 stages, and rows holding inf / nan (with the all-zero row, the quantizer's
general path)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import aq_internal as A
from tests.modules_util import to_f32_numpy
from tests.test_gemm_aq import SHAPES, _inputs

pytestmark = pytest.mark.gpu

from sdnq_amd import ops  # noqa: E402

GEOMETRIES = [A.GEO_64x128, A.GEO_32x256]
EXTRA_SHAPES = [(33, 256, 128), (47, 520, 128), (95, 248, 640), (1024, 1280, 640), (1023, 1272, 1280), (161, 1536, 1280), (2048, 1280, 1280)]


@pytest.fixture
def geometry(request):
    A.set_geometry(request.param)
    yield request.param
    A.set_geometry(-1)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES + EXTRA_SHAPES)
@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_int8_each_geometry_equals_two_launch_route_and_oracle(geometry, shape, dtype, gpu_device):
    m, n, k = shape
    x, b, sb, bias = _inputs(m, n, k, dtype, m + 7 * n + k, gpu_device)
    xq_o, xs_o, _ = O.rowquant(x.float().cpu().numpy(), "int8")
    for with_bias in (True, False):
        bb = bias if with_bias else None
        y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bb, dtype)
        y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bb, dtype)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y1), _bits(y2)), (geometry, shape, dtype, with_bias, int((_bits(y1) != _bits(y2)).sum()))
        ref = O.scaled_mm("int8", xq_o, b.cpu().numpy(), xs_o.reshape(-1), sb.cpu().numpy(), bb.float().cpu().numpy() if with_bias else None,
                          "bf16" if dtype == torch.bfloat16 else "f16")
        assert np.array_equal(to_f32_numpy(y1), ref), (geometry, shape, dtype, with_bias)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(64, 128, 128), (333, 1288, 1152), (1024, 1280, 1280), (1000, 640, 640), (47, 520, 128)])
@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_fp8_each_geometry_equals_two_launch_route(geometry, shape, dtype, gpu_device):
    m, n, k = shape
    x, _, sb, bias = _inputs(m, n, k, dtype, 3 * m + n + k, gpu_device)
    g = torch.Generator().manual_seed(k)
    b = (torch.randn(n, k, generator=g) * 50).clamp(-448, 448).to(torch.float8_e4m3fn).to(gpu_device)
    for with_bias in (True, False):
        bb = bias if with_bias else None
        y2, _, _ = ops.linear_w8a8(ops.MM_FP8, x, b, sb, bb, dtype)
        y1 = ops.linear_w8a8_fused(ops.MM_FP8, x, b, sb, bb, dtype)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y1), _bits(y2)), (geometry, shape, dtype, with_bias, int((_bits(y1) != _bits(y2)).sum()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(70, 264, 128), (130, 640, 640), (1024, 1280, 1280)])
@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_inf_nan_and_zero_rows_take_the_general_path_identically(geometry, shape, dtype, gpu_device):
    """Rows whose scale is 0, inf or nan leave the lean quantizer for the general one; a wave holding one sends its other rows there
    too.  Same bits as the two-launch route everywhere (nan payloads included), and as the oracle in every row it defines finitely."""
    m, n, k = shape
    x, b, sb, bias = _inputs(m, n, k, dtype, 11 * m + n + k, gpu_device)
    x[5, 3] = float("inf")
    x[6, k - 1] = float("-inf")
    x[9, 0] = float("nan")
    x[m - 1, k // 2] = float("inf")
    x[m - 2] = 0
    y2, xq, xs = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, dtype)
    y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y1), _bits(y2)), (geometry, shape, dtype, int((_bits(y1) != _bits(y2)).sum()))
    ordinary = torch.isfinite(x.float()).all(dim=1).cpu().numpy()
    with np.errstate(all="ignore"):
        xq_o, xs_o, _ = O.rowquant(x.float().cpu().numpy()[ordinary], "int8")
    ref = O.scaled_mm("int8", xq_o, b.cpu().numpy(), xs_o.reshape(-1), sb.cpu().numpy(), bias.float().cpu().numpy(),
                      "bf16" if dtype == torch.bfloat16 else "f16")
    assert np.array_equal(to_f32_numpy(y1)[ordinary], ref), (geometry, shape, dtype)


@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_strided_rows_and_repeatability_each_geometry(geometry, gpu_device):
    """A row-strided activation view (ldx > K) and six back-to-back runs (a mis-ordered LDS-DMA / barrier shows up as run-to-run noise)."""
    m, n, k = 1024, 1280, 1280
    x, b, sb, bias = _inputs(m, n, k, torch.bfloat16, 5, gpu_device)
    wide = torch.zeros(m, k + 256, dtype=torch.bfloat16, device=gpu_device)
    wide[:, :k] = x
    xv = wide[:, :k]
    ref, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, torch.bfloat16)
    for _ in range(6):
        y = ops.linear_w8a8_fused(ops.MM_I8, xv, b, sb, bias, torch.bfloat16)
        assert torch.equal(_bits(y), _bits(ref))
