"""Dynamic quantization on the MI355X: the fused loss kernel (sdnq_hip_dequant_loss) against the dequantize-then-reduce formulation
for every storage family and layout, its determinism, the HIP search against the reference's fixtures (tests/golden/dyn_*), and a
searched model under accelerate() / torch.compile, and layers whose K is not a multiple of 16."""
import copy

import pytest
import torch

import sdnq_amd
from sdnq_amd import ops
from sdnq_amd import quantizer as Q

from .test_dynamic_host import FIXTURES, check_against_fixture, load_fixture, run_search

pytestmark = pytest.mark.gpu


def quantized(w, dtype, layer="Linear", **kw):
    dq, t = Q.sdnq_quantize_layer_weight(w, layer_class_name=layer, weights_dtype=dtype, **kw)
    return dq, dq.quant_weight(t["weight"], t["scale"], t["zero_point"], t["svd_up"], t["svd_down"])


def torch_loss(qw, ref, had):
    d = ops.dequant(qw, torch.float32, had) - ref.reshape(qw.n, qw.k).float()
    return float((d * d).double().sum())


def check(dq, qw, ref):
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    got = ops.dequant_loss(qw, ref, had)
    want = torch_loss(qw, ref, had)
    assert got == pytest.approx(want, rel=1e-12, abs=0.0)
    return got


INT_DTYPES = ["uint1", "int2", "uint2", "int3", "uint3", "int4", "uint4", "int5", "uint6", "int7", "int8", "uint8", "int9", "uint11",
              "int12", "uint13", "int15", "uint15", "int16"]
FLOAT_DTYPES = ["float2_e1m0fn", "float3_e2m1fnu", "float4_e2m1fn", "float5_e3m1fn", "float6_e3m3fnu", "float7_e4m2fn",
                "float8_e4m3fn", "float8_e5m2", "float8_e4m3fn_sdnq", "float8_e3m5fnu", "float11_e4m6fn", "float16", "float16_e5m10fn"]


@pytest.mark.parametrize("dtype", INT_DTYPES + FLOAT_DTYPES)
@pytest.mark.parametrize("group", [0, -1])
def test_loss_every_storage_family(dtype, group, gpu_device):
    torch.manual_seed(11)
    w = (torch.randn(96, 512, device=gpu_device) * 0.02).to(torch.bfloat16)
    dq, qw = quantized(w, dtype, group_size=group)
    check(dq, qw, w)


@pytest.mark.parametrize("dtype", ["uint1", "uint2", "uint4", "uint8"])
def test_loss_codebook(dtype, gpu_device):
    torch.manual_seed(12)
    w = torch.randn(64, 512, device=gpu_device) * 0.02
    dq, qw = quantized(w, dtype, use_codebook=True)
    check(dq, qw, w)


@pytest.mark.parametrize("dtype,qmm", [("int8", True), ("uint4", False), ("float8_e4m3fn", True), ("int4", True)])
def test_loss_conv_positions_and_direct_layout(dtype, qmm, gpu_device):
    torch.manual_seed(13)
    w = (torch.randn(64, 48, 3, 3, device=gpu_device) * 0.05).to(torch.float16)
    dq, qw = quantized(w, dtype, layer="Conv2d", use_quantized_matmul=qmm)
    check(dq, qw, w)


@pytest.mark.parametrize("svd_dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("qmm", [False, True])
def test_loss_svd(svd_dtype, qmm, gpu_device):
    torch.manual_seed(14)
    w = torch.randn(128, 512, device=gpu_device) * 0.02
    dq, qw = quantized(w, "int4", use_svd=True, svd_rank=16, use_quantized_matmul=qmm, torch_dtype=svd_dtype)
    assert qw.desc.svd_rank == 16
    check(dq, qw, w)


@pytest.mark.parametrize("group", [32, 64, 128, 256, 512])
@pytest.mark.parametrize("dtype", ["int4", "uint8"])
def test_loss_hadamard(group, dtype, gpu_device):
    torch.manual_seed(15)
    w = torch.randn(64, 1536, device=gpu_device) * 0.02
    dq, qw = quantized(w, dtype, use_hadamard=True, hadamard_group_size=group)
    assert dq.use_hadamard and dq.hadamard_group_size == group
    check(dq, qw, w)


def test_loss_16bit_scales_and_zero_points(gpu_device):
    torch.manual_seed(16)
    w = (torch.randn(64, 768, device=gpu_device) * 0.02).to(torch.bfloat16)
    for dtype in ("uint4", "int6", "float5_e2m2fn"):
        dq, qw = quantized(w, dtype, dequantize_fp32=False)
        assert qw.desc.scale_dtype != 0
        check(dq, qw, w)


@pytest.mark.parametrize("ref_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_loss_ref_dtypes_and_strided_ref(ref_dtype, gpu_device):
    torch.manual_seed(17)
    big = (torch.randn(64, 1024 + 64, device=gpu_device) * 0.02).to(ref_dtype)
    ref = big[:, 32:32 + 1024]  # row stride 1088 elements, rows 16-byte aligned
    dq, qw = quantized(ref.contiguous(), "uint4")
    check(dq, qw, ref)
    had_dq, had_qw = quantized(ref.contiguous(), "int8", use_hadamard=True, hadamard_group_size=128)
    check(had_dq, had_qw, ref)


@pytest.mark.parametrize("shape", [(3072, 12288), (12288, 3072)])
def test_loss_large_and_repeatable(shape, gpu_device):
    torch.manual_seed(18)
    w = (torch.randn(*shape, device=gpu_device) * 0.02).to(torch.bfloat16)
    dq, qw = quantized(w, "uint4", group_size=64)
    first = check(dq, qw, w)
    sums = [ops.dequant_loss_sum(qw, w) for _ in range(3)]
    assert all(torch.equal(s.view(torch.int64), sums[0].view(torch.int64)) for s in sums)
    assert float(sums[0]) == first


@pytest.mark.parametrize("name", FIXTURES)
def test_hip_search_reproduces_fixture(name, gpu_device, monkeypatch):
    """The HIP search (quantizer on the GPU, fused loss) makes the reference's choices with its losses.  The SVD fixture's factors
    come from torch.svd_lowrank's random projections, which the device generator draws differently from the host one: there the
    split is computed on the host with the fixture's seed and handed to the device, the rest of the search runs on the GPU."""
    meta, z = load_fixture(name)
    if meta["cfg"].get("use_svd"):
        real = Q.apply_svdquant

        def host_svd(weight, rank=32, steps=8, dtype=None):
            residual, up, down = real(weight.cpu(), rank=rank, steps=steps, dtype=dtype)
            return residual.to(weight.device), up.to(weight.device), down.to(weight.device)

        monkeypatch.setattr(Q, "apply_svdquant", host_svd)
    model, cfg, trace = run_search(meta, z, device=gpu_device)
    # with SVD factors every element is rounded to bfloat16 after the rank-R product is added (dequantizer.py:79-83), so an fp32
    # difference of one unit between the device's dequantization and the host's flips that rounding for some elements and moves
    # the sum far more than it does without SVD: measured up to 8.5e-5 relative on this fixture's candidates.  The choice and the
    # lists are still checked exactly; the fixture keeps every loss 2e-3 away from its threshold.
    check_against_fixture(meta, z, model, cfg, trace, rel=2e-4 if meta["cfg"].get("use_svd") else 1e-5)
    if meta["cfg"].get("use_svd"):
        layer = model.proj
        assert layer.sdnq_dequantizer.use_quantized_matmul and layer.svd_up.is_cuda and layer.svd_up.shape[0] == meta["cfg"]["svd_rank"]


@pytest.mark.parametrize("kind", ["linear_k100", "conv_k36"])
def test_search_on_layers_without_a_kernel_layout(kind, gpu_device):
    """K % 16 != 0: no weight-side kernel lays such a weight out, so the GPU search scores those candidates with the torch
    restatement (as the quantizer quantizes them with torch ops) -- the same choice and losses as the host search."""
    torch.manual_seed(23)
    layer = torch.nn.Linear(100, 64, bias=False) if kind == "linear_k100" else torch.nn.Conv2d(4, 64, 3, bias=False)
    with torch.no_grad():
        layer.weight.mul_(3.0)
    results = {}
    for dev in ("cpu", gpu_device):
        trace = []
        real = Q._candidate_mse

        def spy(dq, data, original, ref):
            out = real(dq, data, original, ref)
            trace.append((dq.weights_dtype, float(out)))
            return out

        Q._candidate_mse = spy
        try:
            lay = copy.deepcopy(layer).to(dev)
            cfg = Q.SDNQConfig(weights_dtype="int2", use_dynamic_quantization=True, dynamic_loss_threshold=2e-3, quant_conv=True,
                               minimum_allowed_numel=0, minimum_allowed_channel_size=0)
            q, cfg = Q.sdnq_quantize_layer(lay, cfg, param_name="layer.weight")
        finally:
            Q._candidate_mse = real
        results[str(dev)] = (q.sdnq_dequantizer.weights_dtype, trace, cfg.modules_dtype_dict)
    (c_dt, c_tr, c_lists), (g_dt, g_tr, g_lists) = results.values()
    assert c_dt == g_dt and c_lists == g_lists and len(c_tr) > 1
    assert [d for d, _ in c_tr] == [d for d, _ in g_tr]
    for (_, a), (_, b) in zip(c_tr, g_tr):
        assert b == pytest.approx(a, rel=1e-5)


def test_searched_model_accelerated_equals_eager_and_compiled(gpu_device):
    """The searched layers' forwards before accelerate() and after it give the same bits; torch.compile of the accelerated layer too."""
    meta, z = load_fixture("model_mixed")
    model, cfg, _ = run_search(meta, z, device=gpu_device)
    torch.manual_seed(19)
    xs = {lname: torch.randn(40, shape[0], device=gpu_device, dtype=torch.bfloat16) for lname, (_k, shape) in meta["geometry"].items()}
    with torch.no_grad():
        before = {lname: getattr(model, lname)(x).clone() for lname, x in xs.items()}
    res = sdnq_amd.accelerate(model)
    assert res.accelerated == len(meta["layers"]) and not res.skipped
    with torch.no_grad():
        for lname, x in xs.items():
            layer = getattr(model, lname)
            after = layer(x)
            assert torch.equal(after, before[lname]), lname
            torch._dynamo.reset()
            assert torch.equal(torch.compile(layer, fullgraph=True)(x), before[lname]), lname
