"""Quantized embeddings on the GPU: SDNQEmbedding.forward (one sdnq_hip_embedding launch) against the reference's forward
(tests/golden/emb_*) and against sdnq_hip_dequant of the whole table, out-of-range ids, the HIP quantizer, accelerate(),
torch.compile and sdnq_amd.capture."""
import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd.support import unsupported_reason

from tests.test_embedding_host import emb_case_names, load_case, quantize_case, stored

pytestmark = pytest.mark.gpu


def f32(t):
    return t.detach().float().cpu().numpy()


def ref_output(meta, z, i):
    tag = meta["tensors"][f"y_{i}"]["dtype"]
    y = stored(z, meta, f"y_{i}")
    return y.float().numpy() if tag in ("bf16", "f16") else y.numpy()


def fixture_layer(meta, z, device):
    """The case's SDNQEmbedding carrying the reference's STORED tensors (the SVD factors are the reference's own draw)."""
    layer = quantize_case(meta, z)
    for key in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
        t = stored(z, meta, key)
        setattr(layer, key, None if t is None else torch.nn.Parameter(t.to(device), requires_grad=False))
    return layer


def assert_contract(got, ref, meta, what):
    """test_dequant_and_requant_vs_golden's contract: bit-exact without SVD / Hadamard; SVD within 1 ulp (16-bit) of the result and
    < 0.1 % of the elements differing (16-bit results: a float32 result compares sums taken in another order); Hadamard within the
    result-dtype bound applied after the rotation."""
    cfg = meta["cfg"]
    if cfg.get("use_hadamard"):
        assert np.all(np.abs(got - ref) <= 2 * np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7 + 1e-6), what
    elif cfg.get("use_svd"):
        assert np.all(np.abs(got - ref) <= np.maximum(np.abs(ref) * 2.0 ** -7, 1e-8)), what
        if meta["dtype"] != "f32":
            assert np.mean(got != ref) < 1e-3, (what, int((got != ref).sum()))
    else:
        assert np.array_equal(got, ref), (what, int((got != ref).sum()))


@pytest.mark.parametrize("name", emb_case_names())
def test_forward_vs_reference_fixture(name, gpu_device):
    meta, z = load_case(name)
    layer = fixture_layer(meta, z, gpu_device)
    assert unsupported_reason(layer) is None
    for i in range(meta["n_ids"]):
        ids = stored(z, meta, f"ids_{i}").to(gpu_device)
        y = layer(ids)
        assert tuple(y.shape) == tuple(ids.shape) + (meta["D"],) and y.dtype == layer.sdnq_dequantizer.result_dtype
        assert_contract(f32(y), ref_output(meta, z, i), meta, (name, i))


def assert_stored_equal(layer, meta, z, name):
    for key in ("weight", "scale", "zero_point"):
        want, got = stored(z, meta, key), getattr(layer, key, None)
        if want is None:
            assert got is None, key
            continue
        got = got.detach().cpu().contiguous()
        assert got.dtype == want.dtype and list(got.shape) == list(want.shape), key
        assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)), (name, key)


@pytest.mark.parametrize("name", [n for n in emb_case_names() if not load_case(n)[0]["cfg"].get("use_svd")])
def test_hip_quantizer_reproduces_fixture(name, gpu_device):
    """The GPU quantizer (Hadamard rotation of the float table, then csrc/quantize.hip or, for 16-bit scales, torch ops) stores the
    reference's bytes.  (SVD cases: the factors are a random low-rank draw -- their layout is checked on the host.)"""
    meta, z = load_case(name)
    assert_stored_equal(quantize_case(meta, z, device=gpu_device), meta, z, name)


@pytest.mark.parametrize("name", [n for n in emb_case_names() if load_case(n)[0]["cfg"].get("use_hadamard")])
def test_hip_quantizer_on_the_host_rotation(name, gpu_device):
    """The quantize-and-pack kernel alone on the Hadamard cases: fed the table rotated on the host (the rotation whose codes the host
    test pins to the reference), it stores the reference's bytes."""
    from sdnq_amd import quantizer as Q
    from sdnq_amd.quant_utils import apply_hadamard
    from tests.test_embedding_host import float_layer
    meta, z = load_case(name)
    cfg = dict(meta["cfg"])
    w, use, g = apply_hadamard(float_layer(meta, z).weight.detach(), cfg.pop("hadamard_group_size", 256))
    assert use and g == meta["deq"]["hadamard_group_size"]
    cfg.pop("use_hadamard")
    _, tensors = Q.sdnq_quantize_layer_weight(w.to(gpu_device), layer_class_name="Embedding", **cfg)
    layer = torch.nn.Module()
    for key, t in tensors.items():
        setattr(layer, key, t)
    assert_stored_equal(layer, meta, z, name)


def table_layer(V, D, cfg, device, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(V, D, device=device, dtype=dtype)
    with torch.no_grad():
        emb.weight.normal_(0.0, 0.02)
    layer, _ = sdnq_amd.sdnq_quantize_layer(emb, sdnq_amd.SDNQConfig(quant_embedding=True, **cfg))
    assert isinstance(layer, sdnq_amd.layers.SDNQEmbedding) and unsupported_reason(layer) is None
    return layer


def whole_table(layer):
    dq = layer.sdnq_dequantizer
    return dq(layer.weight, layer.scale, zero_point=layer.zero_point, svd_up=layer.svd_up, svd_down=layer.svd_down)


def check_vs_table(layer, table, ids):
    got, want = layer(ids), table[ids.long()]
    assert got.shape == want.shape
    if layer.sdnq_dequantizer.use_hadamard:  # the fused rotation sums as sdnq_hip_hadamard does; held to the golden bound anyway
        g, w = f32(got), f32(want)
        assert np.all(np.abs(g - w) <= 2 * np.maximum(np.abs(w), 1e-30) * 2.0 ** -7 + 1e-6)
    else:
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


CONFIGS = {
    "int8": dict(weights_dtype="int8", group_size=-1),
    "int4_g32": dict(weights_dtype="int4", group_size=32),
    "uint4": dict(weights_dtype="uint4"),
    "fp8": dict(weights_dtype="float8_e4m3fn", group_size=-1),
    "int4_had": dict(weights_dtype="int4", use_hadamard=True),
    "int8_svd": dict(weights_dtype="int8", group_size=-1, use_svd=True, svd_rank=16),
}


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_gather_equals_whole_table_dequant_t5(cfg, gpu_device):
    V, D = 32128, 4096
    layer = table_layer(V, D, CONFIGS[cfg], gpu_device)
    table = whole_table(layer)
    g = torch.Generator(device=gpu_device).manual_seed(1)
    for n in (1, 8192):
        ids = torch.randint(0, V, (n,), device=gpu_device, generator=g)
        ids[0] = V - 1
        check_vs_table(layer, table, ids)
        check_vs_table(layer, table, ids.to(torch.int32))
    ids2 = torch.randint(0, V, (64, 32), device=gpu_device, generator=g)
    check_vs_table(layer, table, ids2[:, ::2])  # non-contiguous ids
    check_vs_table(layer, table, ids2.t())


@pytest.mark.parametrize("cfg", ["int4_g32", "int4_had"])
def test_gather_equals_whole_table_dequant_262144x3840(cfg, gpu_device):
    V, D = 262144, 3840
    layer = table_layer(V, D, CONFIGS[cfg], gpu_device)
    table = whole_table(layer)
    g = torch.Generator(device=gpu_device).manual_seed(2)
    for n in (1, 8192):
        ids = torch.randint(0, V, (n,), device=gpu_device, generator=g)
        check_vs_table(layer, table, ids)
        check_vs_table(layer, table, ids.to(torch.int32))
    del table


@pytest.mark.parametrize("cfg", ["int8", "int4_had", "int8_svd"])
def test_out_of_range_ids_give_nan_rows(cfg, gpu_device):
    V, D = 1000, 512
    layer = table_layer(V, D, CONFIGS[cfg], gpu_device)
    ids = torch.tensor([3, -1, V, 0, V + 7, -(2 ** 40), V - 1, 2 ** 40], device=gpu_device)
    bad = (ids < 0) | (ids >= V)
    y = layer(ids)
    assert torch.isnan(y[bad]).all()
    assert not torch.isnan(y[~bad]).any()
    assert torch.equal(y[~bad], layer(ids[~bad]))
    y32 = layer(ids.clamp(-(2 ** 31), 2 ** 31 - 1).to(torch.int32))
    assert torch.isnan(y32[bad]).all() and torch.equal(y32[~bad], y[~bad])


def test_embed_scale_and_16bit_scales(gpu_device):
    layer = table_layer(4096, 1024, dict(weights_dtype="int4"), gpu_device)
    ids = torch.randint(0, 4096, (4, 33), device=gpu_device)
    base = layer(ids)
    layer.scalar_embed_scale = 3840 ** 0.5
    scaled = layer(ids)
    assert torch.equal(scaled, (base.float() * float(3840 ** 0.5)).to(torch.bfloat16))  # result.mul_(embed_scale) in bf16 op-math
    del layer.scalar_embed_scale
    # with a Hadamard rotation the scale multiplies the ROTATED, rounded rows last (result.mul_(embed_scale) after dequantize)
    had = table_layer(4096, 1024, dict(weights_dtype="int4", use_hadamard=True, hadamard_group_size=256), gpu_device)
    base_h = had(ids)
    check_vs_table(had, whole_table(had), ids)
    had.scalar_embed_scale = 3840 ** 0.5
    assert torch.equal(had(ids), (base_h.float() * float(3840 ** 0.5)).to(torch.bfloat16))
    sdnq_amd.apply_sdnq_options_to_model(torch.nn.Sequential(layer), dequantize_fp32=False)
    assert layer.scale.dtype == torch.bfloat16 and unsupported_reason(layer) is None
    check_vs_table(layer, whole_table(layer), ids)


def test_accelerate_repoints_foreign_embedding(gpu_device):
    meta, z = load_case("int4_g32_bf16")
    layer = fixture_layer(meta, z, gpu_device)

    def foreign_forward(self, input):  # what a model built by another package carries
        raise AssertionError("the foreign forward must not run after accelerate()")

    layer.forward_func = foreign_forward
    model = torch.nn.Sequential(layer)
    res = sdnq_amd.accelerate(model)
    assert res.accelerated == 1 and not res.skipped
    assert layer.forward_func is sdnq_amd.embedding.quantized_embedding_forward
    ids = stored(z, meta, "ids_1").to(gpu_device)
    assert np.array_equal(f32(model(ids)), ref_output(meta, z, 1))


class TinyLM(torch.nn.Module):
    def __init__(self, emb, proj):
        super().__init__()
        self.emb, self.proj = emb, proj

    def forward(self, ids):
        return self.proj(self.emb(ids))


def test_compile_and_capture_equal_eager(gpu_device):
    emb = table_layer(2048, 512, dict(weights_dtype="int4", use_hadamard=True), gpu_device)
    lin = torch.nn.Linear(512, 256, device=gpu_device, dtype=torch.bfloat16)
    proj, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", use_quantized_matmul=True))
    model = TinyLM(emb, proj).eval()
    ids = torch.randint(0, 2048, (2, 40), device=gpu_device)
    with torch.no_grad():
        eager = model(ids)
        torch._dynamo.reset()
        compiled = torch.compile(model, fullgraph=True)(ids)
        assert torch.equal(compiled, eager)
        step = sdnq_amd.capture(model, ids)
        for _ in range(2):
            ids2 = torch.randint(0, 2048, (2, 40), device=gpu_device)
            assert torch.equal(step(ids2), model(ids2))
