"""GPU parity of the one-launch w8a8 Linear on the tall tile geometry of csrc/gemm_aq.hip (K <= 640): 2 = the 64 x 128 tile on a 2-slot
weight ring, two workgroups per CU (what the shape rule picks at 4096 x 640 x 640).

Every output bit equals the two-launch route (sdnq_hip_rowquant + sdnq_hip_scaled_mm) and the CPU oracle -- equality, no tolerance.
Shapes: M below one tile and ragged against 64- and 128-row blocks; N of one ragged column tile up to five column tiles; K of one
stage, of fewer stages than ring slots + 1, and the full five-stage image; more tiles than resident workgroup slots (a second round,
and a last walk group of fewer row blocks); one model-size problem by shape."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import aq_internal as A
from tests.modules_util import to_f32_numpy
from tests.test_gemm_aq import _inputs

pytestmark = pytest.mark.gpu

from sdnq_amd import _lib, ops  # noqa: E402

GEO_TALL = 2
GEOMETRIES = [GEO_TALL]
SHAPES = [(m, n, k) for m in (33, 160, 200) for n in (8, 136, 640) for k in (128, 384, 640)]
# more tiles than the 256-CU part holds at once: 65 x 8 = 520 tiles of 64 x 128 on 512 slots
MULTI_ROUND = {GEO_TALL: (4160, 1024, 128)}


@pytest.fixture
def geometry(request):
    A.set_geometry(request.param)
    yield request.param
    A.set_geometry(-1)


def _bits(t):
    return t.view(torch.int16)


def _oracle(x, b, sb, bias, dtype):
    xq_o, xs_o, _ = O.rowquant(x.float().cpu().numpy(), "int8")
    return O.scaled_mm("int8", xq_o, b.cpu().numpy(), xs_o.reshape(-1), sb.cpu().numpy(), None if bias is None else bias.float().cpu().numpy(),
                       "bf16" if dtype == torch.bfloat16 else "f16")


def _check(geometry, x, b, sb, bias, dtype, tag):
    for bb in (bias, None):
        y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bb, dtype)
        y1 = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bb, dtype)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y1), _bits(y2)), (geometry, tag, dtype, bb is not None, int((_bits(y1) != _bits(y2)).sum()))
        assert np.array_equal(to_f32_numpy(y1), _oracle(x, b, sb, bb, dtype)), (geometry, tag, dtype, bb is not None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_tall_geometry_equals_two_launch_route_and_oracle(geometry, shape, dtype, gpu_device):
    m, n, k = shape
    assert A.plan(ops.MM_I8, m, n, k, 256)["geometry"] == geometry
    x, b, sb, bias = _inputs(m, n, k, dtype, m + 7 * n + k, gpu_device)  # (holds an all-zero row, a row of ties, a half-zero row)
    _check(geometry, x, b, sb, bias, dtype, shape)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(200, 136, 640), (160, 640, 384)])
@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_tall_nan_inf_zero_rows_and_strided_input(geometry, shape, dtype, gpu_device):
    """A row holding a NaN (its amax is re-taken over the other elements), rows holding +-inf, an all-zero row, all read through a
    row-strided view (ldx > K): the bits of the two-launch route everywhere, the oracle's in every row it defines finitely."""
    m, n, k = shape
    x, b, sb, bias = _inputs(m, n, k, dtype, 11 * m + n + k, gpu_device)
    x[5, 3] = float("inf")
    x[6, k - 1] = float("-inf")
    x[9, 0] = float("nan")
    x[m - 1, k // 2] = float("nan")
    x[m - 2] = 0
    wide = torch.full((m, k + 64), 7.0, dtype=dtype, device=gpu_device)
    wide[:, :k] = x
    xv = wide[:, :k]
    y2, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, dtype)
    y1 = ops.linear_w8a8_fused(ops.MM_I8, xv, b, sb, bias, dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y1), _bits(y2)), (geometry, shape, dtype, int((_bits(y1) != _bits(y2)).sum()))
    ordinary = torch.isfinite(x.float()).all(dim=1).cpu()
    ref = _oracle(x[ordinary.to(gpu_device)], b, sb, bias, dtype)
    assert np.array_equal(to_f32_numpy(y1)[ordinary.numpy()], ref), (geometry, shape, dtype)


@pytest.mark.parametrize("geometry", GEOMETRIES, indirect=True)
def test_tall_more_tiles_than_resident_slots(geometry, gpu_device):
    """A second round of workgroups and a last walk group of one row block (65 row blocks in groups of 8)."""
    m, n, k = MULTI_ROUND[geometry]
    p = A.plan(ops.MM_I8, m, n, k, 256)
    assert p["geometry"] == geometry and p["prefetch_room"] < 0 and p["tiles_m"] % p["group_m"] == 1
    x, b, sb, bias = _inputs(m, n, k, torch.bfloat16, 3, gpu_device)
    _check(geometry, x, b, sb, bias, torch.bfloat16, (m, n, k))


def test_model_size_problem_by_shape_is_repeatable(gpu_device):
    """4096 x 640 x 640, unforced: the route is on, and three runs give the two-launch route's bits."""
    m, n, k = 4096, 640, 640
    A.set_geometry(-1)
    assert _lib.load().sdnq_hip_linear_w8a8_fused_supported(0, 1, 1, m, n, k) == 1
    assert A.plan(ops.MM_I8, m, n, k, 256)["geometry"] == GEO_TALL
    x, b, sb, bias = _inputs(m, n, k, torch.bfloat16, 17, gpu_device)
    ref, _, _ = ops.linear_w8a8(ops.MM_I8, x, b, sb, bias, torch.bfloat16)
    for _ in range(3):
        y = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, torch.bfloat16)
        assert torch.equal(_bits(y), _bits(ref))
