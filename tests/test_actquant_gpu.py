"""ops.act_rowquant (csrc/actquant.hip) against the float64 restatement of its formula and against the row quantizer on its own y;
SDNQFusedActivation in front of a w8a8 SDNQLinear against the same layer with identity reuse disabled.

The bound of the accuracy check, per element, with u = 2^-24:   |y - ref| <= ulp_T(|ref|) / 2 + C u |a| max(1, |b|)
C is the float32 error constant of the activation forms, derived in the head comment of csrc/actquant.hip: GELU(erf) 24, GELU(tanh) 7, SiLU 6."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C = {"gelu": 24, "gelu_tanh": 7, "silu": 6}
M = 5  # one more than a workgroup's four rows
# one lane; a ragged second pass; the largest register form; the smallest LDS form; the smallest recompute sweep (past 16384)
NS = (8, 520, 4096, 4104, 16392)
LAYOUTS = ("ungated", "halves", "padded")
# every N with every activation and layout; the dtype and the matmul dtype rotate through the product
CASES = [(act, lay, n, ("bf16", "f16")[(i + j + k) % 2], ("int8", "fp8")[(i + j + k) // 2 % 2])
         for i, act in enumerate(C) for j, lay in enumerate(LAYOUTS) for k, n in enumerate(NS)]


def _reference(act, a, b):
    a = a.detach().cpu().to(torch.float64)
    if act == "gelu":
        g = 0.5 * a * (1 + torch.special.erf(a / math.sqrt(2)))
    elif act == "gelu_tanh":
        g = 0.5 * a * (1 + torch.tanh(math.sqrt(2 / math.pi) * (a + 0.044715 * a ** 3)))
    else:
        g = a / (1 + torch.exp(-a))
    b = torch.ones_like(a) if b is None else b.detach().cpu().to(torch.float64)
    return g * b, a.abs() * b.abs().clamp_min(1)


def _half_ulp(v, dtype):  # half the spacing of `dtype` at magnitude v (float64), the subnormal spacing below the smallest normal
    fi = torch.finfo(dtype)
    return 0.5 * torch.exp2(torch.floor(torch.log2(v.clamp_min(fi.tiny)))) * fi.eps


def _check_y(act, y, a, b, what):
    ref, mag = _reference(act, a, b)
    bound = _half_ulp(ref.abs(), y.dtype) + C[act] * 2.0 ** -24 * mag
    ratio = ((y.cpu().to(torch.float64) - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"actquant accuracy {what}: worst |y - ref| / bound = {ratio:.4f}")
    assert torch.isfinite(y.float()).all() and ratio <= 1.0


def _operands(layout, n, dtype, dev):
    g = torch.Generator().manual_seed(n)
    a, b = 2 * torch.randn(M, n, generator=g), 1.5 * torch.randn(M, n, generator=g)
    a[0, :4] = torch.tensor([0.0, -0.0, 12.0, -12.0])
    a[2, -4:] = torch.tensor([-12.0, 12.0, -0.0, 0.0])
    a[3], b[3] = 0.0, 0.0  # an all-zero row: scale 0
    if layout == "ungated":
        return a.to(dtype).to(dev), None
    if layout == "halves":  # one [M][2N] projection output: the value first, the gate second
        h = torch.cat([b, a], 1).to(dtype).to(dev)
        return h[:, n:], h[:, :n]
    pad = torch.zeros(M, 8)
    return torch.cat([a, pad], 1).to(dtype).to(dev)[:, :n], torch.cat([b, pad, pad], 1).to(dtype).to(dev)[:, :n]


@pytest.mark.parametrize("act, layout, n, dtype, mm_name", CASES)
def test_act_rowquant(act, layout, n, dtype, mm_name):
    from sdnq_amd import ops
    code = {"gelu": ops.ACT_GELU, "gelu_tanh": ops.ACT_GELU_TANH, "silu": ops.ACT_SILU}[act]
    mm = ops.mm_code(mm_name)
    a, b = _operands(layout, n, {"bf16": torch.bfloat16, "f16": torch.float16}[dtype], torch.device("cuda:0"))
    y, xq, xs = ops.act_rowquant(a, b, code, mm)

    def same(got, want):
        return all(torch.equal(t.view(torch.uint8), r.view(torch.uint8)) for t, r in zip(got, want))

    # 1. the codes are the row quantizer's for that y;  2. stored or not
    assert same((xq, xs), ops.rowquant(y, mm, 0)[:2])
    y0, xq0, xs0 = ops.act_rowquant(a, b, code, mm, want_y=False)
    assert y0 is None and same((xq0, xs0), (xq, xs))
    # 3. y against the float64 formula; signed zeros and the all-zero row
    _check_y(act, y, a, b, f"{act} {layout} {dtype} N={n}")
    if b is None:
        assert y[0, :2].view(torch.int16).tolist() == [0, -32768]
    assert not y[3].any() and not xq[3].view(torch.uint8).any() and xs[3].item() == 0.0
    assert same(ops.act_rowquant(a, b, code, None)[:1], (y,))  # the activation alone: the same y


class GEGLU(torch.nn.Module):  # the shape of diffusers' class
    def __init__(self, k, n):
        super().__init__()
        self.proj = torch.nn.Linear(k, 2 * n, dtype=torch.bfloat16)

    def forward(self, x):
        h, gate = self.proj(x).chunk(2, dim=-1)
        return h * torch.nn.functional.gelu(gate)


class MLP(torch.nn.Module):
    def __init__(self, k, n, consumer):
        super().__init__()
        self.gate_proj, self.up_proj = torch.nn.Linear(k, n, dtype=torch.bfloat16), torch.nn.Linear(k, n, dtype=torch.bfloat16)
        self.down_proj, self.act_fn = consumer, torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


@pytest.mark.parametrize("shape", ["plain", "proj", "mlp"])
def test_consumer_runs_on_the_parked_codes(shape):
    import sdnq_amd
    from sdnq_amd import linear as L
    from sdnq_amd.activations import SDNQFusedActivation
    torch.manual_seed(3)
    dev, rows, k, n = torch.device("cuda:0"), 32, 64, 256  # 32 rows: the fewest the w8a8 route takes
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    consumer = sdnq_amd.sdnq_quantize_layer(torch.nn.Linear(n, n).to(torch.bfloat16), cfg)[0]
    module = {"plain": lambda: torch.nn.GELU(approximate="tanh"), "proj": lambda: GEGLU(k, n), "mlp": lambda: MLP(k, n, consumer)}[shape]()
    fused = SDNQFusedActivation(module).to(dev).eval()  # (no dtype cast: the consumer keeps its float32 scales)
    consumer = consumer.to(dev)
    x = torch.randn(rows, n if shape == "plain" else k).to(torch.bfloat16).to(dev)
    L.clear_activation_cache()
    with torch.no_grad():
        if shape == "mlp":  # the consumer is the wrapped module's own down_proj
            seeded = fused(x)
            a, b = module.gate_proj(x), module.up_proj(x)
            y = L._ts.act_cache.entries[-1][0]
        else:
            y = fused(x)
            seeded = consumer(y)
            a, b = (x, None) if shape == "plain" else (module.proj(x)[:, n:], module.proj(x)[:, :n])
        entry = L._ts.act_cache.entries[-1]
        assert entry[0] is y and entry[5] is fused and entry[6][0] and len(L._ts.act_cache.entries) == 1  # parked, hit, nobody quantized again
        _check_y({"plain": "gelu_tanh", "proj": "gelu", "mlp": "silu"}[shape], y, a, b, f"wrapper {shape}")
        L.clear_activation_cache()
        with L.identity_reuse_disabled():
            plain = consumer(y)
    L.clear_activation_cache()
    assert torch.equal(seeded.view(torch.int16), plain.view(torch.int16))
