"""Input gradients through frozen quantized Conv1d / Conv2d layers on the GPU: sdnq_hip_im2col_bwd against the torch restatement of its
index map (tests/conv_grad_util.py, itself checked against torch.nn.grad.conv{1,2}d_input on the CPU), QuantizedConvInputGrad against a
float64 backward-data convolution with the CPU oracle's dequantized weight, an adapter graph, the slabs, the paths that must stay what
they were, the scratch buffers and a captured backward.

Tolerance of the fixture gradient checks: the standing float-GEMM bound of tests/test_gpu_parity.py (assert_close_float) -- fp32
accumulation, ONE rounding to the layer dtype.  No Hadamard doubling: the weight is un-rotated before the product."""
import math

import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import linear as L, ops, scratch, training as T
from tests import conv_grad_util as U
from tests.golden_util import ConvCase, conv_case_names
from tests.modules_util import to_f32_numpy
from tests.test_gpu_parity import assert_close_float

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
INT8 = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, quant_conv=True)


def accepted_fixtures():
    """The Conv1d / Conv2d fixtures the predicate accepts, judged on CPU copies of the modules (static facts only)."""
    return [n for n in conv_case_names() if T.input_grad_unsupported_reason(ConvCase(n).torch_module(None), convs=True) is None]


ACCEPTED = accepted_fixtures()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_the_predicate_accepts_every_zero_padded_conv1d_and_conv2d_fixture():
    """40 conv fixtures: 7 are Conv3d, one pads by reflection; the other 32 -- every storage format, SVD, Hadamard, 16-bit scales, groups 2
    and 4, stride 2 -- are served."""
    names = conv_case_names()
    rejected = sorted(set(names) - set(ACCEPTED))
    assert len(names) == 40 and len(ACCEPTED) == 32, (len(names), len(ACCEPTED))
    assert all(n.startswith("conv3d_") or n == "conv2d_int8_qmm_dil_reflect_bf16" for n in rejected), rejected
    for must in ("conv2d_int8_svd16_qmm_bf16", "conv2d_g2_int8_had_qmm_bf16", "conv1d_g4_uint4_noqmm_f32", "conv2d_int8_qmm_s2_f16_nobias",
                 "conv2d_g2_int8_qmm_bf16_lpscale", "conv2d_g4_fp8_qmm_bf16_nobias", "conv1d_int8_qmm_bf16"):
        assert must in ACCEPTED, must


@pytest.mark.parametrize("geom", U.GEOMETRIES, ids=U.geometry_id)
def test_im2col_bwd_moves_the_bits_of_the_restatement(geom, gpu_device):
    """Whole U, then a row window that starts and ends inside an image row, written into a buffer whose tail is a canary."""
    kernel, stride, padding, dilation, in_hw = U.as_2d(geom)
    ho, wo = U.out_hw(in_hw, kernel, stride, padding, dilation)
    total = U.BATCH * in_hw[0] * in_hw[1]
    row0 = in_hw[1] + 2 if in_hw[0] > 1 else 5
    rows = total - row0 - 3
    assert row0 % in_hw[1] and (row0 + rows) % in_hw[1] and rows > 0
    for cout in U.C_OUTS:
        kc = kernel[0] * kernel[1] * cout
        for dt in DTYPES:
            dy = torch.randn(U.BATCH, cout, ho, wo, generator=torch.Generator().manual_seed(cout)).to(dt)
            dy[0, 1, 0, 0] = -0.0                                             # moved, not recomputed: the sign of a zero survives
            dyg = dy.to(gpu_device)
            for groups in (1, 2):
                want = U.unfold_bwd(dy, in_hw, kernel, stride, padding, dilation, groups)
                got = ops.im2col_bwd(dyg, in_hw, kernel, stride, padding, dilation, groups=groups)
                what = (U.geometry_id(geom), cout, dt, groups)
                assert got.shape == (total, kc) and torch.equal(bits(got).cpu(), bits(want)), (what, int((bits(got).cpu() != bits(want)).sum()))
                buf = torch.full((rows + 2, kc), 3.0, device=gpu_device, dtype=dt)       # rows `rows`, `rows + 1`: the guard behind out
                win = ops.im2col_bwd(dyg, in_hw, kernel, stride, padding, dilation, row0=row0, rows=rows, out=buf, groups=groups)
                assert win.data_ptr() == buf.data_ptr() and win.shape == (rows, kc)
                assert torch.equal(bits(win).cpu(), bits(want[row0:row0 + rows])), (what, "window")
                assert bool((buf[rows:] == 3.0).all()), (what, "guard")


def oracle_weight(c):
    """[C_out][C_in / groups][*kernel] in float64: the CPU oracle's dequantized weight (SVD product added, Hadamard rotation undone) --
    ConvCase.oracle_module serves every conv fixture, so no fixture falls back to ops.dequant."""
    return torch.from_numpy(c.oracle_module().dequantize().astype(np.float64)).reshape(tuple(c.deq["original_shape"]))


ROUTED = [(n, "gather") for n in ACCEPTED] + [(n, "col2im") for n in ACCEPTED if ConvCase(n).conv["groups"] == 1]


@pytest.mark.parametrize("name,route", ROUTED, ids=lambda v: v)
def test_grad_input_on_conv_fixtures(name, route, gpu_device, monkeypatch):
    """Forward under grad: the bits of the plain call.  Backward: x.grad against conv{1,2}d_input in float64 on the oracle's weight, every
    input of the fixture, on each route the layer can take (grouped layers gather); grad_bias where the fixture has a bias; the frozen
    tensors get nothing."""
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", route)
    assert T._takes_col2im_route(ConvCase(name).conv["groups"], 9, (1, 1), 10 ** 6) == (route == "col2im")
    c = ConvCase(name)
    mod = c.torch_module(gpu_device)
    assert T.input_grad_unsupported_reason(mod, convs=True) is None
    cv = c.conv
    w64 = oracle_weight(c)
    dt = mod.sdnq_dequantizer.result_dtype
    conv_input = torch.nn.grad.conv1d_input if cv["nd"] == 1 else torch.nn.grad.conv2d_input
    for i in c.inputs():
        x = c.torch_tensor(f"x_{i}", device=gpu_device)
        with torch.no_grad():
            plain = mod(x.clone())
        xg = x.clone().requires_grad_()
        y = T.quantized_conv_input_grad(mod, xg)
        assert y.grad_fn is not None and y.dtype == plain.dtype and torch.equal(bits(y.detach()), bits(plain)), (name, i)
        dy = (torch.randn(y.shape, generator=torch.Generator().manual_seed(1000 + i)) * 0.02).to(dt).to(gpu_device)
        y.backward(dy)
        assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == dt and xg.grad.is_contiguous()
        ref = conv_input(tuple(x.shape), w64, dy.double().cpu(), stride=tuple(cv["stride"]), padding=tuple(cv["padding"]),
                         dilation=tuple(cv["dilation"]), groups=cv["groups"]).numpy()
        got = to_f32_numpy(xg.grad).astype(np.float64)
        print(name, route, i, c.tag, "max err / scale", float(np.abs(got - ref).max() / np.abs(ref).max()), "rel l2",
              float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
        assert_close_float(got, ref, c.tag, (name, route, i, "grad_input"))
    if cv["groups"] > 1 and not mod.sdnq_dequantizer.use_hadamard:   # a plain grouped layer decodes row slabs of its stored tensors
        slabs = mod.__dict__["_sdnq_conv_grad_slabs"][1]
        assert slabs is not None and len(slabs) == cv["groups"] and all(q.n == c.N // cv["groups"] for q in slabs), name
    if mod.bias is not None:
        mod.bias.requires_grad_()
        xg = x.clone().requires_grad_()
        T.quantized_conv_input_grad(mod, xg).backward(dy)
        want = dy.sum(dim=[0] + list(range(2, dy.ndim)))
        assert torch.equal(bits(mod.bias.grad), bits(want.to(mod.bias.dtype))) and mod.weight.grad is None and mod.scale.grad is None


def quantized(module, device, **cfg):
    layer, _ = sdnq_amd.sdnq_quantize_layer(module, sdnq_amd.SDNQConfig(**{**INT8, **cfg}))
    assert getattr(layer, "sdnq_dequantizer", None) is not None
    return layer.to(device)


def seeded_conv(cin, cout, k, device, dtype=torch.bfloat16, seed=0, cfg=None, **kw):
    torch.manual_seed(seed)
    return quantized(torch.nn.Conv2d(cin, cout, k, **kw).to(dtype), device, **(cfg or {}))


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=lambda d: TAG[d])
def test_adapter_graph_trains_through_a_quantized_conv(dtype, gpu_device):
    """x -> A (float32 1x1 conv 8 -> 32, trainable) -> cast to the layer dtype -> quantized 3x3 conv 32 -> 64 -> the pixels flattened ->
    quantized Linear 64 -> 48 (enable_input_grad-wrapped) -> sum(y * dY).  A.weight.grad against the twin graph on ops.dequant's weights in
    float64.  Without convs=True the conv cuts the graph and that gradient is None.

    Bound: between dY and A.weight.grad lie TWO roundings to the layer dtype, one after the other -- grad_input of the Linear, then
    grad_input of the conv, which reads the first one's rounded values; A itself is a float32 master adapter, and torch's conv backward of
    it accumulates in float32.  Two independent relative errors of the size the standing float-GEMM bound allows for one rounding add in
    quadrature, so rel-L2 <= sqrt(2) x its limit (bf16 2e-3, f16 5e-4) and, for the largest element, max err / scale <= 2 x its 2 ulp."""
    torch.manual_seed(3)
    a = torch.nn.Conv2d(8, 32, 1).to(gpu_device)
    conv = seeded_conv(32, 64, 3, gpu_device, dtype=dtype, seed=1, padding=1)
    torch.manual_seed(2)
    lin = quantized(torch.nn.Linear(64, 48).to(dtype), gpu_device)

    class Adapted(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.conv, self.lin = a, conv, lin

        def forward(self, x):
            h = self.conv(self.a(x).to(dtype))
            return self.lin(h.permute(0, 2, 3, 1).reshape(-1, h.shape[1]))

    model = Adapted()
    x = torch.randn(2, 8, 12, 12, device=gpu_device)
    dy = (torch.randn(2 * 12 * 12, 48, device=gpu_device) * 0.02).to(dtype)
    assert sdnq_amd.accelerate(model) == 2
    with pytest.warns(UserWarning, match="still cut the autograd graph"):
        assert sdnq_amd.enable_input_grad(model) == 1          # the default: the conv still cuts the graph
    assert model(x).grad_fn is None and a.weight.grad is None
    assert sdnq_amd.enable_input_grad(model, convs=True) == 2
    y = model(x)
    assert y.grad_fn is not None and y.dtype == dtype
    (y * dy).sum().backward()
    assert a.weight.grad is not None
    wc = ops.dequant(L._state(conv).qw, dtype, 0).double().view(64, 32, 3, 3)
    wl = ops.dequant(L._state(lin).qw, dtype, 0).double()
    a64 = a.weight.detach().double().requires_grad_()
    h64 = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x.double(), a64, a.bias.detach().double()), wc, conv.bias.detach().double(), padding=1)
    y64 = torch.nn.functional.linear(h64.permute(0, 2, 3, 1).reshape(-1, 64), wl, lin.bias.detach().double())
    (y64 * dy.double()).sum().backward()
    got, ref = to_f32_numpy(a.weight.grad).astype(np.float64), a64.grad.cpu().numpy()
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    l2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print("conv adapter", TAG[dtype], "max err / scale", err, "rel l2", l2)
    ulp, l2_one = {torch.bfloat16: (2.0 ** -8, 2e-3), torch.float16: (2.0 ** -11, 5e-4)}[dtype]
    assert err <= 2 * 2 * ulp, ("A.weight.grad", TAG[dtype], "max err / scale", err)
    assert l2 <= math.sqrt(2.0) * l2_one, ("A.weight.grad", TAG[dtype], "rel l2", l2)


def test_slabs_change_no_bit(gpu_device, monkeypatch):
    """2 x 32 x 24 x 24 through a 3x3 conv to 64 channels: U is 1152 rows of 1152 bytes.  0.4 MB slabs hold 364 rows -- four slabs, every
    edge inside an image row (364 = 15 * 24 + 4) -- and give the bits of the one-slab run.  The col2im route cuts between images: its
    float32 matrix is 576 x 288 x 4 = 663552 bytes per image, so 0.4 MB slabs hold one image each."""
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", "gather")
    conv = seeded_conv(32, 64, 3, gpu_device, padding=1)
    x = torch.randn(2, 32, 24, 24, device=gpu_device).to(torch.bfloat16)
    dy = (torch.randn(2, 64, 24, 24, device=gpu_device) * 0.02).to(torch.bfloat16)

    def grad():
        xg = x.clone().requires_grad_()
        T.quantized_conv_input_grad(conv, xg).backward(dy)
        return xg.grad
    monkeypatch.delenv("SDNQ_HIP_CONV_GRAD_SLAB_MB", raising=False)
    assert T._slab_rows(1152, 1152) == 1152
    one = grad()
    calls = []
    real = ops.im2col_bwd
    monkeypatch.setattr(ops, "im2col_bwd", lambda *a, **k: (calls.append((k["row0"], k["rows"])), real(*a, **k))[1])
    monkeypatch.setenv("SDNQ_HIP_CONV_GRAD_SLAB_MB", "0.4")
    T.release_scratch()
    many = grad()
    assert calls == [(0, 364), (364, 364), (728, 364), (1092, 60)] and all(r0 % 24 for r0, _ in calls[1:])
    assert T.scratch_bytes(gpu_device) == 64 * 288 * 2 + 364 * 1152
    assert torch.equal(bits(many), bits(one)), int((bits(many) != bits(one)).sum())
    T.release_scratch()
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", "col2im")
    images = []
    real_c2i = ops.col2im
    monkeypatch.setattr(ops, "col2im", lambda cols, bias, dt, batch, *a, **k: (images.append(batch), real_c2i(cols, bias, dt, batch, *a, **k))[1])
    per_image = grad()
    assert images == [1, 1] and T.scratch_bytes(gpu_device) == 64 * 288 * 2 + 663552
    monkeypatch.delenv("SDNQ_HIP_CONV_GRAD_SLAB_MB")
    T.release_scratch()
    whole = grad()
    assert images == [1, 1, 2] and T.scratch_bytes(gpu_device) == 64 * 288 * 2 + 2 * 663552
    assert torch.equal(bits(per_image), bits(whole)), int((bits(per_image) != bits(whole)).sum())
    T.release_scratch()


def test_no_grad_paths_are_what_they_were(gpu_device):
    conv = seeded_conv(32, 64, 3, gpu_device, padding=1)
    model = torch.nn.Sequential(conv)
    assert sdnq_amd.accelerate(model) == 1
    x = torch.randn(2, 32, 12, 12, device=gpu_device).to(torch.bfloat16)
    inference = conv.forward_func
    before = [model(x).clone() for _ in range(3)][-1]
    assert sdnq_amd.enable_input_grad(model, convs=True) == 1
    inner = conv.forward_func._sdnq_inference_forward
    assert inner is inference
    for _ in range(2):
        with torch.no_grad():
            y = model(x)
        assert y.grad_fn is None and torch.equal(bits(y), bits(before))
        y = model(x)                                    # gradients on, an input that does not require grad
        assert y.grad_fn is None and torch.equal(bits(y), bits(before))
        xg = x.clone().requires_grad_()
        with torch.no_grad():
            y = model(xg)
        assert y.grad_fn is None and torch.equal(bits(y), bits(before))
        y = model(xg)
        assert y.grad_fn is not None and torch.equal(bits(y.detach()), bits(before))
    assert sdnq_amd.enable_input_grad(model, enabled=False) == 1 and conv.forward_func is inference
    y = model(x.clone().requires_grad_())
    assert y.grad_fn is None and torch.equal(bits(y), bits(before))


def test_scratch_is_the_largest_operand_plus_the_largest_unfolded_slab(gpu_device, monkeypatch):
    monkeypatch.delenv("SDNQ_HIP_CONV_GRAD_SLAB_MB", raising=False)
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", "gather")
    c1 = seeded_conv(32, 64, 3, gpu_device, seed=1, padding=1)       # operand 64 * 288 * 2 = 36864 B, U 288 x 576 x 2 = 331776 B
    c2 = seeded_conv(64, 48, 3, gpu_device, seed=2, padding=1)       # operand 48 * 576 * 2 = 55296 B, U 288 x 432 x 2 = 248832 B
    model = torch.nn.Sequential(c1, c2)
    assert sdnq_amd.accelerate(model) == 2 and sdnq_amd.enable_input_grad(model, convs=True) == 2
    x = torch.randn(2, 32, 12, 12, device=gpu_device).to(torch.bfloat16)
    T.release_scratch()
    assert T.scratch_bytes(gpu_device) == 0
    model(x.clone().requires_grad_()).float().sum().backward()
    operand, unfolded = 55296, 331776
    assert T.scratch_bytes(gpu_device) == operand + unfolded and "decoded" not in scratch.held(gpu_device)
    ptrs = [b.data_ptr() for b in scratch.held(gpu_device).values()]
    assert len(ptrs) == 2
    model(x.clone().requires_grad_()).float().sum().backward()
    assert [b.data_ptr() for b in scratch.held(gpu_device).values()] == ptrs                        # reused, not regrown
    # a capped slab caps the third buffer: 0.125 MB = 131072 B hold 113 rows of c1's U (1152 B each) or 151 of c2's (864 B each)
    T.release_scratch()
    monkeypatch.setenv("SDNQ_HIP_CONV_GRAD_SLAB_MB", "0.125")
    model(x.clone().requires_grad_()).float().sum().backward()
    assert T.scratch_bytes(gpu_device) == operand + max(131072 // 1152 * 1152, 131072 // 864 * 864)
    monkeypatch.delenv("SDNQ_HIP_CONV_GRAD_SLAB_MB")
    T.release_scratch()
    model(x.clone().requires_grad_()).float().sum().backward()
    # a Hadamard layer brings the second buffer, of the size of the first
    had = seeded_conv(64, 32, 3, gpu_device, seed=3, padding=1, cfg=dict(use_hadamard=True, hadamard_group_size=64))
    assert had.sdnq_dequantizer.use_hadamard
    hx = torch.randn(1, 64, 6, 6, device=gpu_device).to(torch.bfloat16).requires_grad_()
    T.quantized_conv_input_grad(had, hx).float().sum().backward()
    assert T.scratch_bytes(gpu_device) == 2 * operand + unfolded
    T.release_scratch()
    assert T.scratch_bytes(gpu_device) == 0


@pytest.mark.parametrize("route", ("gather", "col2im"))
def test_a_captured_backward_replays_to_the_same_bits(route, gpu_device, monkeypatch):
    """One eager backward sizes the buffers; the backward is then captured into a graph (nothing in it synchronises with the host or
    allocates scratch) and replayed twice."""
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", route)
    conv = seeded_conv(32, 64, 3, gpu_device, stride=2, padding=1)
    x = torch.randn(2, 32, 16, 16, device=gpu_device).to(torch.bfloat16)
    xg = x.clone().requires_grad_()
    y = T.quantized_conv_input_grad(conv, xg)
    dy = (torch.randn(y.shape, device=gpu_device) * 0.02).to(torch.bfloat16)
    y.backward(dy)
    eager = xg.grad.clone()
    ctx = type("Ctx", (), {"layer": conv, "input_shape": x.shape, "needs_input_grad": (False, True, False), "bias_dtype": None})()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        T.QuantizedConvInputGrad.backward(ctx, dy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gi = T.QuantizedConvInputGrad.backward(ctx, dy)[1]
    graph.replay()
    torch.cuda.synchronize()
    first = gi.clone()
    gi.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(first), bits(gi)) and torch.equal(bits(first), bits(eager))
    T.release_scratch()


def test_the_unfolded_buffer_refuses_to_grow_while_capturing(gpu_device, monkeypatch):
    """The rule of the first two buffers; no capture is opened for it: the check reads torch.cuda.is_current_stream_capturing."""
    T.release_scratch()
    assert T._scratch_unfolded(gpu_device, torch.bfloat16, 4096).numel() == 4096
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert T._scratch_unfolded(gpu_device, torch.bfloat16, 2048).numel() == 4096          # fits: served
    with pytest.raises(ops._lib.SdnqHipError, match="before capturing"):
        T._scratch_unfolded(gpu_device, torch.bfloat16, 8192)
    monkeypatch.undo()
    T.release_scratch()
