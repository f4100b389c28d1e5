"""Transposed convolutions on the GPU: sdnq_hip_dequant_convt and sdnq_hip_col2im against exact references, the HIP quantizer path, every
fixture through the module forward (eager, `output_size=`, under a captured graph) and accelerate() on a mixed module.

Error measure of the forward tests: distance(a, ref) = max |a - ref| / max |ref| against a float64 F.conv_transposeNd of the fixture's
reference-dequantized weight, computed on the CPU (tests/convt_util.ref64).  Bound: the rule of tests/test_optim_gpu.py::float_bound --
twice the distance of the reference's own stored output from the same restatement, plus one ulp of the storage dtype (REL_ULP): the
operations are the same, only the summation order differs.

Measured on an MI355X (profiles/convt_accuracy.md holds the table): the kernel's distance equals the reference's own to four digits on
every 16-bit fixture (bf16 1.6e-3 .. 3.0e-3, f16 2.7e-4 .. 3.0e-4: the one rounding at the store dominates both) and is 3.199e-7 against the
reference's 3.233e-7 (bound 7.658e-7) on the float32 fixture -- so the float32 fixture needs no other bound.
"""
import pytest
import torch

from tests import convt_util as U
from tests.optim_util import REL_ULP, distance

pytestmark = pytest.mark.gpu


def measured(name, got):
    """(distance of `got`, distance of the reference's stored output, bound) for fixture `name`; printed before anything is asserted."""
    meta, t = U.load(name)
    r = U.ref64(name)
    d, d_ref = distance(got.cpu(), r), distance(t["y"], r)
    bound = 2.0 * d_ref + REL_ULP[meta["dtype"]]
    print(f"convt {name}: kernel {d:.3e} reference {d_ref:.3e} bound {bound:.3e}")
    return d, d_ref, bound


@pytest.mark.parametrize("name", U.NAMES)
def test_dequant_convt_bit_equal(name, gpu_device):
    """sdnq_hip_dequant_convt against the reference's dequantized weight permuted to the operand layout [groups, P, C_in / groups]: bit
    equal.  The 16-bit-scale fixture is held to the same rule tests/test_gpu_parity.py:191-194 applies to sdnq_hip_dequant on 16-bit
    scales (no Hadamard, no SVD: np.array_equal)."""
    from sdnq_amd import ops
    meta, t = U.load(name)
    groups = meta["layer"].get("groups", 1)
    shape = meta["deq"]["original_shape"]
    kprod = 1
    for d in shape[2:]:
        kprod *= d
    dev = lambda x: None if x is None else x.to(gpu_device)  # noqa: E731
    qw = ops.make_convt_weight(meta["deq"]["weights_dtype"], dev(t["weight"]), dev(t["scale"]), dev(t.get("zero_point")), shape[0],
                               shape[1] * kprod, kprod)
    got = ops.dequant_convt(qw, U.TORCH_DT[meta["dtype"]], groups)
    want = U.operand_layout(t["w_deq"], groups)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(U.bits(got), U.bits(want)), int((U.bits(got) != U.bits(want)).sum())
    # ... and the dequantizer's own call returns the reference's tensor
    mod = U.stored_module(meta, t, gpu_device)
    w = mod.sdnq_dequantizer(mod.weight, mod.scale, mod.zero_point, None, None)
    assert tuple(w.shape) == tuple(shape) and torch.equal(U.bits(w), U.bits(t["w_deq"]))


# geometry of every fixture (batch, channels, input, kernel, stride, padding, dilation, output_padding) plus one whose output_padding
# rows and columns receive no tap at all: k 1, stride 3, output_padding 2 -> two of every three outputs are bias only
GEOMETRIES = {n: None for n in U.NAMES if n not in ("2d_int5_bf16", "2d_int8_lpscale_bf16")}  # (those two repeat the first's geometry)
GEOMETRIES["bias_only_rows"] = dict(batch=2, channels=5, size=(3, 4), kernel=(1, 1), stride=(3, 3), padding=(0, 0), dilation=(1, 1), output_padding=(2, 2))


def _geometry(name):
    g = GEOMETRIES[name]
    if g is not None:
        return g
    meta, t = U.load(name)
    nd, kw = meta["nd"], U.layer_kwargs(meta)
    tup = lambda v: (v,) * nd if isinstance(v, int) else tuple(v)  # noqa: E731
    return dict(batch=t["x"].shape[0], channels=meta["cout"], size=tuple(t["x"].shape[2:]), kernel=tup(meta["k"]), stride=tup(kw.get("stride", 1)),
                padding=tup(kw.get("padding", 0)), dilation=tup(kw.get("dilation", 1)), output_padding=U.output_padding(meta, t))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_col2im_exact_sums(name, gpu_device):
    """Integer-valued cols in [0, 3] and bias in [0, 7]: at most 64 taps reach an output (k 16 / stride 8: 2; 4 x 4 / stride 2: 4; 3^3 with
    strides (1, 2, 2): 12), so every output is an integer <= 3 * 64 + 7 < 2^8 -- exact in float32, bfloat16 and float16 alike -- and must
    equal the float64 restatement (conv_transpose of an identity-like fold, written with torch on the CPU) bit for bit."""
    from sdnq_amd import ops
    g = _geometry(name)
    nd = len(g["size"])
    kprod = 1
    for k in g["kernel"]:
        kprod *= k
    positions = 1
    for s in g["size"]:
        positions *= s
    b, c = g["batch"], g["channels"]
    gen = torch.Generator().manual_seed(len(name) * 7919 + c)
    cols = torch.randint(0, 4, (b * positions, c * kprod + 8), generator=gen).float()  # 8 spare columns: a leading dimension > C * prod(k)
    bias = torch.randint(0, 8, (c,), generator=gen).float()
    # float64 restatement: out[b, co] = bias[co] + conv_transpose(cols as [B, co * kprod + kpos, *in], one-hot weight) -- the fold written
    # as a grouped transposed convolution whose weight [C * kprod, 1, *k] has a single 1 at kernel position kpos
    x = cols[:, : c * kprod].double().reshape(b, *g["size"], c * kprod).movedim(-1, 1)
    w = torch.zeros(c * kprod, 1, *g["kernel"], dtype=torch.float64)
    w.view(c, kprod, kprod)[:, torch.arange(kprod), torch.arange(kprod)] = 1.0
    taps = U.FUNC[nd](x, w, None, g["stride"], g["padding"], g["output_padding"], c * kprod, g["dilation"])  # [B, C * kprod, *out]
    want = taps.reshape(b, c, kprod, *taps.shape[2:]).sum(2) + bias.double().view(1, c, *([1] * nd))
    assert float(want.max()) < 256 and float(want.min()) >= 0
    if name == "bias_only_rows":
        assert bool((want[:, :, -1] == bias.double().view(1, c, 1)).all())  # the last row: output_padding only
    out_size = tuple(want.shape[2:])
    cols_d = cols.to(gpu_device)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        got = ops.col2im(cols_d, bias.to(dt).to(gpu_device), dt, b, c, g["size"], out_size, g["kernel"], g["stride"], g["padding"], g["dilation"])
        assert got.dtype == dt and tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.cpu().double(), want), (name, dt, int((got.cpu().double() != want).sum()))
    got = ops.col2im(cols_d, None, torch.float32, b, c, g["size"], out_size, g["kernel"], g["stride"], g["padding"], g["dilation"])
    assert torch.equal(got.cpu().double(), want - bias.double().view(1, c, *([1] * nd)))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("m", [7, 200])
def test_linear_float_f32out_exact(dt, m, gpu_device):
    """The float32-storing GEMM entry on exact-sum inputs (integers in [-4, 4], K = 64: |sum| <= 1024), through the few-row kernel (m = 7)
    and the matrix-core tiles (m = 200), on a column view with a leading dimension: equal to the float64 product, and the columns
    outside the view untouched."""
    from sdnq_amd import ops
    gen = torch.Generator().manual_seed(m)
    x = torch.randint(-4, 5, (m, 96), generator=gen).to(dt)
    w = torch.randint(-4, 5, (40, 64), generator=gen).to(dt)
    out = torch.full((m, 56), -7.0, device=gpu_device)
    ops.linear_float_f32_into(x.to(gpu_device)[:, 16:80], w.to(gpu_device), out, 8)
    want = x[:, 16:80].double() @ w.double().t()
    assert torch.equal(out[:, 8:48].cpu().double(), want)
    assert bool((out[:, :8] == -7.0).all()) and bool((out[:, 48:] == -7.0).all())


@pytest.mark.parametrize("name", U.NAMES)
def test_hip_quantizer_reproduces_the_reference(name, gpu_device):
    """sdnq_quantize_layer on GPU tensors: the fixture's stored tensors bit for bit.  Every fixture's format (int8, uint8, fp8, packed
    int5 and uint4; the column and the square grouped layout) goes through the HIP row quantizer with the reduction axis moved last."""
    meta, t = U.load(name)
    q = U.quantize_here(meta, t, gpu_device)
    assert U.deq_fields(q.sdnq_dequantizer) == meta["deq"]
    for key in ("weight", "scale", "zero_point"):
        mine = getattr(q, key)
        if key not in t:
            assert mine is None
            continue
        assert mine.is_cuda and mine.dtype == t[key].dtype and tuple(mine.shape) == tuple(t[key].shape), key
        assert torch.equal(U.bits(mine), U.bits(t[key])), (key, int((U.bits(mine) != U.bits(t[key])).sum()))


@pytest.mark.parametrize("name", U.NAMES)
def test_module_forward(name, gpu_device):
    """Each fixture through the module's forward (with `output_size=` where the fixture has one), and unbatched."""
    meta, t = U.load(name)
    mod = U.stored_module(meta, t, gpu_device)
    x = t["x"].to(gpu_device)
    y = mod(x, output_size=list(meta["output_size"])) if meta["output_size"] else mod(x)
    assert y.dtype == x.dtype and tuple(y.shape) == tuple(t["y"].shape) and y.is_contiguous()
    d, d_ref, bound = measured(name, y)
    assert d <= bound, (name, d, d_ref, bound)
    if meta["output_size"]:
        assert torch.equal(mod(x, list(meta["output_size"])), y)  # positional, as torch's own forward takes it
    else:
        y1 = mod(x[0])  # unbatched input [C_in, *in]
        assert tuple(y1.shape) == tuple(y.shape[1:]) and torch.equal(y1, y[0])


def test_forward_under_a_captured_graph(gpu_device):
    """Nothing in the forward synchronises with the host: the first fixture captured into a graph, replayed twice with equal bits."""
    name = U.NAMES[0]
    meta, t = U.load(name)
    mod = U.stored_module(meta, t, gpu_device)
    x = t["x"].to(gpu_device)
    eager = mod(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mod(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = mod(x)
    graph.replay()
    torch.cuda.synchronize()
    first = y.clone()
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, y) and torch.equal(first, eager)
    d, d_ref, bound = measured(name, first)
    assert d <= bound


class _Mixed(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Linear(64, 64)
        self.conv = torch.nn.Conv2d(64, 64, 3, padding=1)
        self.up = torch.nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1)
        self.up_svd = torch.nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1)

    def forward(self, x):
        h = self.conv(self.proj(x.movedim(1, -1)).movedim(-1, 1))
        return self.up(h)


def test_accelerate_on_a_mixed_module(gpu_device):
    """accelerate() on a module holding a Linear, a Conv2d and a ConvTranspose2d layer: all three are re-pointed at this package's
    forwards and the output stays within the forward tests' bound (twice the distance of a bfloat16 CPU run of the same three torch
    functions, plus one ulp) against a float64 run of the dequantized layers; a transposed
    layer carrying SVD factors lands in `res.skipped` with the predicate's sentence and keeps the forward it came with."""
    import warnings
    import sdnq_amd
    from sdnq_amd.support import unsupported_reason
    torch.manual_seed(5)
    model = _Mixed().to(torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", quant_conv=True, minimum_allowed_numel=1024)
    model = sdnq_amd.sdnq_post_load_quant(model, torch_dtype=torch.bfloat16, quantization_config=cfg).to(gpu_device)
    came_with = lambda self, input, output_size=None: input  # noqa: E731  (stands for another package's forward)
    model.up_svd.svd_up = torch.nn.Parameter(torch.zeros(64, 8, device=gpu_device, dtype=torch.bfloat16), requires_grad=False)
    model.up_svd.svd_down = torch.nn.Parameter(torch.zeros(8, 512, device=gpu_device, dtype=torch.bfloat16), requires_grad=False)
    for m in (model.proj, model.conv, model.up, model.up_svd):
        m.forward_func = came_with
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = sdnq_amd.accelerate(model)
    assert res.accelerated == 3 and [n for n, _ in res.skipped] == ["up_svd"]
    assert res.skipped[0][1] == unsupported_reason(model.up_svd) and "SVD factors on transposed convolutions" in res.skipped[0][1]
    assert any("up_svd" in str(w.message) for w in seen)
    assert model.up_svd.forward_func is came_with
    for m in (model.proj, model.conv, model.up):
        assert m.forward_func.__module__.startswith("sdnq_amd")
    assert model.up.forward_func.__name__ == "quantized_conv_transpose_2d_forward"
    x = torch.randn(2, 64, 6, 5).to(torch.bfloat16)
    y = model(x.to(gpu_device))
    # float64 restatement of the three layers on their dequantized weights, rounding to bfloat16 where the model's tensors do
    F = torch.nn.functional
    deq = lambda m: m.sdnq_dequantizer(m.weight, m.scale, m.zero_point, None, None).double().cpu()  # noqa: E731
    b = lambda m: m.bias.double().cpu()  # noqa: E731
    h = F.linear(x.double().movedim(1, -1), deq(model.proj), b(model.proj)).to(torch.bfloat16).double().movedim(-1, 1)
    h = F.conv2d(h, deq(model.conv), b(model.conv), padding=1).to(torch.bfloat16).double()
    want = F.conv_transpose2d(h, deq(model.up), b(model.up), stride=2, padding=1)
    # the reference side of the bound: the same three torch functions in bfloat16 on the CPU, on the same dequantized weights
    lo = lambda v: v.to(torch.bfloat16)  # noqa: E731
    hr = F.linear(x.movedim(1, -1), lo(deq(model.proj)), lo(b(model.proj))).movedim(-1, 1)
    hr = F.conv2d(hr, lo(deq(model.conv)), lo(b(model.conv)), padding=1)
    y_ref = F.conv_transpose2d(hr, lo(deq(model.up)), lo(b(model.up)), stride=2, padding=1)
    d, d_ref = distance(y.cpu(), want), distance(y_ref, want)
    bound = 2.0 * d_ref + REL_ULP["bf16"]  # the forward tests' rule (tests/test_optim_gpu.py::float_bound)
    print(f"convt accelerate mixed: kernel {d:.3e} reference {d_ref:.3e} bound {bound:.3e}")
    assert tuple(y.shape) == (2, 32, 12, 10) and d <= bound
