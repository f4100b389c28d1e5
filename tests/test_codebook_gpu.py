"""Codebook layers (use_codebook=True) on the MI355X: the HIP Lloyd-Max quantizer, dequantize, re-quantize (int8 / fp8 / uint8), the
4-bit table GEMM and every forward against the reference's fixtures (tests/golden/cb_*), plus accelerate(), torch.compile and
sdnq_amd.capture on codebook models."""
import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import ops
from sdnq_amd.support import unsupported_reason
from tests.test_codebook_host import cb_case_names, load_case, quantize_case, stored
from tests.test_embedding_gpu import assert_contract
from tests.test_gpu_parity import assert_close_float

pytestmark = pytest.mark.gpu

TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def f32(t):
    return t.detach().float().cpu().numpy()


def ref_f32(z, meta, key):
    return stored(z, meta, key).float().numpy()


def fixture_layer(meta, z, device):
    """The case's layer carrying the reference's STORED tensors (the SVD factors are the reference's own draw)."""
    layer = quantize_case(meta, z)
    for key in ("weight", "scale", "zero_point", "svd_up", "svd_down", "bias"):
        t = stored(z, meta, key)
        setattr(layer, key, None if t is None else torch.nn.Parameter(t.to(device), requires_grad=False))
    return layer


def bytes_of(t):
    return t.detach().contiguous().cpu().view(torch.uint8).numpy()


@pytest.mark.parametrize("name", [n for n in cb_case_names() if not load_case(n)[0]["cfg"].get("use_svd")])
def test_hip_quantizer_reproduces_fixture(name, gpu_device):
    """sdnq_hip_quantize_codebook (the GPU branch of the quantizer) stores the reference's codes and levels byte for byte."""
    meta, z = load_case(name)
    layer = quantize_case(meta, z, device=gpu_device)
    for key in ("weight", "scale"):
        want = stored(z, meta, key)
        got = getattr(layer, key)
        assert got.is_cuda and list(got.shape) == list(want.shape), (name, key)
        assert np.array_equal(bytes_of(got), bytes_of(want)), (name, key, int((bytes_of(got) != bytes_of(want)).sum()))
    assert layer.zero_point is None


@pytest.mark.parametrize("wd,gs", [("uint4", 0), ("uint8", 0), ("uint2", 128)])
def test_hip_quantizer_equals_host_quantizer_3072(wd, gs, gpu_device):
    from sdnq_amd import quantizer as Q
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(3072, 3072, generator=g) * 0.02).to(torch.bfloat16)
    cfg = dict(layer_class_name="Linear", weights_dtype=wd, group_size=gs, use_codebook=True, use_quantized_matmul=True)
    _, host = Q.sdnq_quantize_layer_weight(w, **cfg)
    _, dev = Q.sdnq_quantize_layer_weight(w.to(gpu_device), **cfg)
    assert dev["scale"].is_cuda
    for key in ("weight", "scale"):
        assert host[key].shape == dev[key].shape and np.array_equal(bytes_of(host[key]), bytes_of(dev[key])), (wd, key)


@pytest.mark.parametrize("name", [n for n in cb_case_names() if load_case(n)[0]["kind"] != "embedding"])
def test_dequant_and_requant_vs_reference(name, gpu_device):
    meta, z = load_case(name)
    layer = fixture_layer(meta, z, gpu_device)
    dq = layer.sdnq_dequantizer
    wd = dq(layer.weight, layer.scale, zero_point=layer.zero_point, svd_up=layer.svd_up, svd_down=layer.svd_down,
            skip_quantized_matmul=dq.use_quantized_matmul)
    assert tuple(wd.shape) == tuple(meta["tensors"]["w_dequant"]["shape"])
    assert_contract(f32(wd), ref_f32(z, meta, "w_dequant"), meta, (name, "dequant"))
    if dq.use_quantized_matmul:
        rq = dq.re_quantize_matmul(layer.weight, layer.scale, zero_point=layer.zero_point)
        keys = ["requant_weight", "requant_scale"] + (["requant_zero_point"] if len(rq) > 2 else [])
        assert len(rq) == len(keys)
        for key, got in zip(keys, rq):
            want = stored(z, meta, key)
            assert list(got.shape) == list(want.shape) and got.dtype == want.dtype, (name, key)
            assert np.array_equal(bytes_of(got), bytes_of(want)), (name, key, int((bytes_of(got) != bytes_of(want)).sum()))


@pytest.mark.parametrize("name", cb_case_names())
def test_forward_vs_reference_fixture(name, gpu_device):
    meta, z = load_case(name)
    layer = fixture_layer(meta, z, gpu_device)
    dq = layer.sdnq_dequantizer
    assert unsupported_reason(layer) is None
    for i in range(meta["n_inputs"]):
        x = stored(z, meta, f"x_{i}").to(gpu_device)
        y = layer(x)
        ref = ref_f32(z, meta, f"y_{i}")
        assert tuple(y.shape) == ref.shape and y.dtype == dq.result_dtype, (name, i)
        if meta["kind"] == "embedding":
            assert_contract(f32(y), ref, meta, (name, i))
            continue
        m = x.numel() // x.shape[-1] if meta["kind"] == "linear" else 32
        exact = (dq.use_quantized_matmul and m >= 32 and dq.quantized_matmul_dtype in ("int8", "uint8") and not dq.use_hadamard
                 and layer.svd_up is None)
        if exact:
            assert np.array_equal(f32(y), ref), (name, i, int((f32(y) != ref).sum()))
        else:
            assert_close_float(f32(y), ref, meta["dtype"], (name, i), hadamard=dq.use_hadamard)


def _uint4_layer(device, n=256, k=1024, **cfg):
    torch.manual_seed(11)
    lin = torch.nn.Linear(k, n, device=device, dtype=torch.bfloat16)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="uint4", use_codebook=True, use_quantized_matmul=True,
                                                                      **cfg))
    return layer


def test_lut4_tables_and_w4_gemm_on_codebooks(gpu_device, monkeypatch):
    """The 4-bit table route serves codebook weights: the table kernel writes the general re-quantizer's bytes, and
    sdnq_hip_scaled_mm_w4 on the codebook's tables equals sdnq_hip_scaled_mm on the re-quantized operand bit for bit."""
    layer = _uint4_layer(gpu_device)
    qw = layer.sdnq_dequantizer.quant_weight(layer.weight, layer.scale)
    wq, ws = ops.requant(qw, ops.MM_I8)
    monkeypatch.setenv("SDNQ_HIP_REQUANT_LUT", "0")
    wq_gen, ws_gen = ops.requant(qw, ops.MM_I8)
    monkeypatch.delenv("SDNQ_HIP_REQUANT_LUT")
    assert torch.equal(wq, wq_gen) and torch.equal(ws, ws_gen)
    lut, ws_lut = ops.lut4_build(qw, ops.MM_I8)
    assert torch.equal(ws_lut, ws)
    g = torch.Generator(device=gpu_device).manual_seed(3)
    for m in (1, 16, 64):
        a = torch.randint(-127, 128, (m, 1024), device=gpu_device, dtype=torch.int8, generator=g)
        sa = torch.rand(m, device=gpu_device, generator=g) * 0.01
        want = ops.scaled_mm(ops.MM_I8, a, wq, sa, ws, layer.bias, torch.bfloat16)
        got = ops.scaled_mm_w4(a, layer.weight, lut, sa, ws, layer.bias, torch.bfloat16)
        assert torch.equal(got, want), m


def test_per_call_and_float_modes_equal_cached(gpu_device, monkeypatch):
    """Per-call mode (SDNQ_HIP_CACHE_WEIGHTS=0: re-quantization or the gemm_w4 route on every call) and the skinny float path give the
    cached mode's outputs."""
    import sdnq_amd.linear as L
    layer = _uint4_layer(gpu_device)
    x = torch.randn(48, 1024, device=gpu_device, dtype=torch.bfloat16)
    xs = torch.randn(4, 1024, device=gpu_device, dtype=torch.bfloat16)
    with torch.no_grad():
        cached, small = layer(x), layer(xs)
        monkeypatch.setattr(L, "CACHE_WEIGHTS", False)
        layer.__dict__.pop("_sdnq_hip_state", None)
        for _ in range(2):  # (the second call takes the per-call pipeline with known row scales)
            assert torch.equal(layer(x), cached)
        assert torch.equal(layer(xs), small)
    dq = layer.sdnq_dequantizer
    wd = dq(layer.weight, layer.scale, skip_quantized_matmul=True)
    assert_close_float(f32(small), f32(torch.nn.functional.linear(xs.float(), wd.float(), layer.bias.float())), "bf16", "skinny")


class CodebookNet(torch.nn.Module):
    def __init__(self, device):
        super().__init__()
        self.emb = torch.nn.Embedding(512, 256)
        self.a = torch.nn.Linear(256, 512)
        self.b = torch.nn.Linear(512, 256)
        self.conv = torch.nn.Conv2d(64, 64, 3, padding=1)
        self.to(device=device, dtype=torch.bfloat16)

    def forward(self, ids, img):
        h = self.emb(ids)
        h = self.b(torch.nn.functional.gelu(self.a(h)))
        return h, self.conv(img)


@pytest.mark.parametrize("wd", ["uint4", "uint8"])
def test_accelerate_compile_and_capture_equal_eager(wd, gpu_device):
    torch.manual_seed(5)
    model = CodebookNet(gpu_device).eval()
    # (group_size 32: an ungrouped codebook conv with a quantized matmul is refused, as the reference's own forward fails on it)
    cfg = sdnq_amd.SDNQConfig(weights_dtype=wd, use_codebook=True, quant_embedding=True, quant_conv=True, group_size=32,
                              use_quantized_matmul=True, use_quantized_matmul_conv=True, minimum_allowed_numel=0)
    model = sdnq_amd.sdnq_post_load_quant(model, quantization_config=cfg)
    res = sdnq_amd.accelerate(model)
    assert res.accelerated == 4 and not res.skipped
    ids = torch.randint(0, 512, (2, 24), device=gpu_device)
    img = torch.randn(2, 64, 8, 8, device=gpu_device, dtype=torch.bfloat16)
    with torch.no_grad():
        eager = model(ids, img)
        torch._dynamo.reset()
        compiled = torch.compile(model, fullgraph=True)(ids, img)
        for c, e in zip(compiled, eager):
            assert torch.equal(c, e)
        step = sdnq_amd.capture(model, ids, img)
        for _ in range(2):
            ids2 = torch.randint(0, 512, (2, 24), device=gpu_device)
            img2 = torch.randn(2, 64, 8, 8, device=gpu_device, dtype=torch.bfloat16)
            for c, e in zip(step(ids2, img2), model(ids2, img2)):
                assert torch.equal(c, e)
