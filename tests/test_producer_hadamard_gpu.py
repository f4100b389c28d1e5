"""The fused producers for rotated consumers (csrc/normquant_had.hip, csrc/actquant_had.hip; ``hadamard_group=`` of
``ops.norm_rowquant`` / ``ops.act_rowquant`` / ``fuse_norms`` / ``fuse_activations``).

The contract has two halves, both bit for bit: ``y`` is what the plain producer writes, and the codes and row scale are what
``ops.rowquant(y, mm, g)`` writes for that ``y``.  A float64 anchor ties the int8 codes to ``R = H . y`` itself.  With u = 2^-24 and eps the row dtype's epsilon:

* the kernel's float32 rotation r32 sums 256 exact products (y times +-1/16) in two stages of 16: |r32 - R| <= S = 2^-20 sum|y| over the
  group (256 u / 16 per unit of |y|, generously);
* the ONE rounding to the row dtype, r = round_T(r32): |r - r32| <= eps / 2 * |r32| <= eps / 2 * (|R| + S);
* the code q = rint(fl(r / xs)), the division correctly rounded: |q xs - r| <= xs / 2 + u |r|, and |r| <= (1 + eps / 2) (|R| + S).

    |xq xs - R| <= xs / 2 + S + (eps / 2 + u (1 + eps / 2)) (|R| + S)

half a code step plus the row-dtype rounding of the rotated value, and what float32 adds to both.  fp8 codes are not anchored this way
(their step is relative); they are held to the row quantizer's bits like everything else."""
import pytest
import torch

import sdnq_amd
from sdnq_amd import linear as L, ops

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (M, K, group).  Group 256 up to 16384 is the matrix-core form: 2, 4, 6, 8 passes in registers (256 / 768, 2048, 3072, 4096), the
# sweep form past them; 16640 and the other groups are the butterfly form: 2, 4, 8 passes (576 / 1024, 2048, 3584) and its sweep (4608)
NORM_SHAPES = [(5, 256, 256), (5, 768, 256), (2, 2048, 256), (3, 3072, 256), (2, 4096, 256), (2, 4352, 256), (2, 12288, 256),
               (2, 16640, 256), (5, 576, 64), (3, 1024, 512), (2, 2048, 64), (2, 3584, 128), (2, 4608, 64)]
# (M, N, group).  The matrix-core form: a row per wave in 2, 4, 6, 8 passes (256 / 768, 2048, 2560, 4096), the row over four waves in
# 6 (4352, 12288) and 8 (16384) passes each; the butterfly form: 2 and 8 passes (576, 2048) and its sweep (4608, and 256 at 16640)
ACT_SHAPES = [(5, 256, 256), (5, 768, 256), (2, 2048, 256), (3, 2560, 256), (2, 4096, 256), (2, 4352, 256), (2, 12288, 256),
              (2, 16384, 256), (2, 16640, 256), (5, 576, 64), (2, 2048, 64), (2, 4608, 64)]
ACTS = {"gelu_tanh": (ops.ACT_GELU_TANH, False), "geglu": (ops.ACT_GELU, True), "gelu_erf": (ops.ACT_GELU, False), "silu": (ops.ACT_SILU, False),
        "swiglu": (ops.ACT_SILU, True)}


def _rows(m, k, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * (0.5 + 2 * torch.rand(m, 1, generator=g)) + torch.randn(m, 1, generator=g)
    x[0] = 0.0                 # an all-zero row: scale 0 behind an activation (and a constant row, var = 0, behind a norm)
    x[1] *= 0.01
    x[1, (5 * k) // 8] = 300.0  # a single huge element: the row's amax by far, the clamp of the fp8 codes
    return x.to(dtype).to(dev)


def _check_codes(y, xq, xs, mm, g):
    rq, rs, _, _ = ops.rowquant(y, mm, g)
    assert torch.equal(xs, rs)
    assert torch.equal(xq.view(torch.uint8), rq.view(torch.uint8))


@pytest.mark.parametrize("m, k, g", NORM_SHAPES)
@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form", ["layernorm_affine", "rmsnorm", "layernorm_adaln"])
def test_norm_rowquant_rotated(gpu_device, form, dtype, mm_name, m, k, g):
    mm = ops.mm_code(mm_name)
    gen = torch.Generator().manual_seed(k + g)
    x = _rows(m, k, dtype, gpu_device, 7 * k + m)
    vec = lambda rows=None: (0.5 * torch.randn(*((k,) if rows is None else (rows, k)), generator=gen)).to(dtype).to(gpu_device)  # noqa: E731
    args = {"layernorm_affine": (ops.NORM_LAYER, EPS, 1 + vec(), vec(), None, None),
            "rmsnorm": (ops.NORM_RMS, EPS, (1 + vec()).float(), None, None, None),
            "layernorm_adaln": (ops.NORM_LAYER, EPS, None, None, vec(1), vec(1))}[form]
    y0, _, _ = ops.norm_rowquant(x, *args, mm)
    y, xq, xs = ops.norm_rowquant(x, *args, mm, hadamard_group=g)
    assert torch.equal(y, y0)
    _check_codes(y, xq, xs, mm, g)
    if form == "rmsnorm":  # (behind a bias or a shift the zero row is not zero)
        assert xs[0].item() == 0.0 and not xq[0].view(torch.uint8).any()


@pytest.mark.parametrize("m, n, g", ACT_SHAPES)
@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form", list(ACTS))
def test_act_rowquant_rotated(gpu_device, form, dtype, mm_name, m, n, g):
    mm = ops.mm_code(mm_name)
    act, gated = ACTS[form]
    if gated:  # the two halves of one [M, 2N] projection output: row-strided views
        h = _rows(m, 2 * n, dtype, gpu_device, 3 * n + m)
        a, b = h[:, n:], h[:, :n]
    else:
        a, b = _rows(m, n, dtype, gpu_device, 5 * n + m), None
    y0, _, _ = ops.act_rowquant(a, b, act, mm)
    y, xq, xs = ops.act_rowquant(a, b, act, mm, hadamard_group=g)
    assert torch.equal(y, y0)
    _check_codes(y, xq, xs, mm, g)
    assert xs[0].item() == 0.0 and not xq[0].view(torch.uint8).any()


def _hadamard(g):
    """H_g for g a power of 4 as the reference builds it: the Kronecker powers of H4, divided by sqrt(g)."""
    h4 = torch.tensor([[1, 1, 1, -1], [1, 1, -1, 1], [1, -1, 1, 1], [-1, 1, 1, 1]], dtype=torch.float64)
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < g:
        h = torch.kron(h, h4)
    return h / g ** 0.5


@pytest.mark.parametrize("producer", ["norm", "act"])
def test_codes_against_the_float64_rotation(gpu_device, producer):
    m, k, g, dtype = 5, 768, 256, torch.bfloat16
    x = _rows(m, k, dtype, gpu_device, 11)
    if producer == "norm":
        y, xq, xs = ops.norm_rowquant(x, ops.NORM_LAYER, EPS, None, None, None, None, ops.MM_I8, hadamard_group=g)
    else:
        y, xq, xs = ops.act_rowquant(x, None, ops.ACT_GELU_TANH, ops.MM_I8, hadamard_group=g)
    y64 = y.double().cpu()
    rot = (y64.view(m, k // g, g) @ _hadamard(g)).view(m, k)
    xs64 = xs.double().cpu()
    eps = torch.finfo(dtype).eps
    u = 2.0 ** -24
    s = 2.0 ** -20 * y64.abs().view(m, k // g, g).sum(-1).repeat_interleave(g, 1)
    bound = xs64 / 2 + s + (eps / 2 + u * (1 + eps / 2)) * (rot.abs() + s)
    err = (xq.double().cpu() * xs64 - rot).abs()
    print(f"{producer}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


def _rotated_linear(k, n, dev):
    torch.manual_seed(0)
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, use_hadamard=True, hadamard_group_size=256)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, cfg)
    dq = layer.sdnq_dequantizer
    assert dq.use_quantized_matmul and dq.use_hadamard and dq.hadamard_group_size == 256
    return layer.to(dev)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("k", [512, 5632], ids=["plain", "long_rows"])  # the inline look-up in front of linear_w8a8 | of linear_call
@pytest.mark.parametrize("producer", ["norm", "act"])
def test_rotated_layer_runs_on_the_parked_codes(gpu_device, producer, k, monkeypatch):
    first = torch.nn.LayerNorm(k).to(torch.bfloat16) if producer == "norm" else torch.nn.GELU(approximate="tanh")
    model = torch.nn.Sequential(first, _rotated_linear(k, 64, gpu_device)).to(gpu_device)
    assert sdnq_amd.accelerate(model) == 1
    fuse, unfuse = ((sdnq_amd.fuse_norms, sdnq_amd.unfuse_norms) if producer == "norm"
                    else (sdnq_amd.fuse_activations, sdnq_amd.unfuse_activations))
    x = _rows(40, k, torch.bfloat16, gpu_device, 5)
    entries = L._ts.act_cache.entries
    with torch.no_grad():
        # un-rotated codes parked: the rotated layer misses them, quantizes for itself and parks its own
        assert fuse(model) == 1
        L.clear_activation_cache()
        ref = model(x).clone()
        assert len(entries) == 2 and entries[0][5] is model[0] and not entries[0][6][0]
        # rotated codes parked: the layer hits them; nobody else quantizes or parks
        assert unfuse(model) == 1 and fuse(model, hadamard_group=256) == 1
        L.clear_activation_cache()
        for name in ("rowquant", "linear_w8a8", "linear_w8a8_ws"):
            monkeypatch.setattr(ops, name, lambda *a, **kw: pytest.fail("the consumer quantized for itself"))
        y = model[0](x)
        entry = entries[-1]
        assert entry[0] is y and entry[5] is model[0] and entry[2][1] == 256 and not entry[6][0]
        out = model[1](y)
        assert entry[6][0] and len(entries) == 1 and entries[-1] is entry
    assert torch.equal(_bits(out), _bits(ref))


def test_unrotated_layer_misses_the_rotated_codes(gpu_device):
    k = 512
    torch.manual_seed(1)
    lin = torch.nn.Linear(k, 64, bias=True).to(torch.bfloat16)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True))
    model = torch.nn.Sequential(torch.nn.LayerNorm(k).to(torch.bfloat16), layer).to(gpu_device)
    assert sdnq_amd.accelerate(model) == 1
    x = _rows(40, k, torch.bfloat16, gpu_device, 6)
    entries = L._ts.act_cache.entries
    with torch.no_grad():
        L.clear_activation_cache()
        ref = model(x).clone()
        assert sdnq_amd.fuse_norms(model, hadamard_group=256) == 1
        L.clear_activation_cache()
        out = model(x)
        assert len(entries) == 2 and entries[0][5] is model[0] and not entries[0][6][0]  # its own codes, not the rotated ones
    L.clear_activation_cache()
    assert torch.equal(_bits(out), _bits(ref))
