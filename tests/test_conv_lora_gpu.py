"""Trainable low-rank adapters on frozen quantized Conv1d / Conv2d layers, end to end on the GPU (sdnq_amd/lora.py, convs=True).

With up = 0 the adapter changes no bit of the layer's output, with and without a graph, on the NCHW route (8 | L) and on the NHWC
fallback.  With random factors each output is held to the DERIVED bound of tests/test_lora_gpu.py (tests/lora_util.bound) on the kernel's
own t and g_t: with e the float64 composition of the same steps, an output that reduces over L terms and is stored in dtype d satisfies

    |got - e| <= ulp_d(e) / 2 + (L + 2) 2^-24 S            S = the sum of the magnitudes of the terms, base value included

y has L = rank; grad_input L = prod(kernel) * rank on top of the base gradient's own rounded value (QuantizedConvInputGrad's bits, taken
from the layer before the adapter goes on); grad_up and grad_down L = M = B * H_out * W_out.  Where ops.lowrank_add cannot add the adapter
term of grad_input in place -- prod(kernel) * rank > 256, or rows that are no 16-byte pieces: 8 does not divide H W on the col2im route
(C_in on the gather route) -- the term is rounded to the layer dtype by ops.linear_float before torch adds it (the documented extra
rounding): such a case adds |scale| * ulp_d(term) / 2 to the bound.  No other tolerance is introduced."""
import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import lora, ops, optim, training as T
from tests import lora_util as L

pytestmark = pytest.mark.gpu

W8A8 = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, use_quantized_matmul_conv=True, quant_conv=True)
UINT4 = dict(weights_dtype="uint4", group_size=64, use_quantized_matmul=False, quant_conv=True)
# name: (module factory, input shape)
LAYERS = {
    "c2d_3x3": (lambda: torch.nn.Conv2d(16, 32, 3, padding=1), (2, 16, 8, 8)),
    "c2d_3x3_s2": (lambda: torch.nn.Conv2d(32, 48, 3, stride=2, padding=1), (1, 32, 9, 9)),    # L = 25: the NHWC fallback; the col2im route
    "c1d_k5": (lambda: torch.nn.Conv1d(16, 32, 5, padding=2), (2, 16, 40)),
    "c2d_1x1": (lambda: torch.nn.Conv2d(64, 64, 1), (1, 64, 8, 8)),
}
# (layer, weights, dtype, rank, forced route of the base gradient or None for the rule's)
CASES = [(n, "w8a8", torch.bfloat16, 16, None) for n in LAYERS] + [(n, "uint4", torch.bfloat16, 16, None) for n in LAYERS] + [
    ("c2d_3x3", "w8a8", torch.float16, 16, None),
    ("c2d_3x3", "w8a8", torch.bfloat16, 16, "gather"),      # the rule sends this layer down the col2im route (128 input positions)
    ("c2d_3x3", "w8a8", torch.bfloat16, 32, "gather"),      # 9 * 32 = 288 > 256: ops.linear_float + add on the NHWC rows
    ("c2d_3x3", "uint4", torch.bfloat16, 32, "col2im"),     # ... and on the NCHW result
]
CFG = {"w8a8": W8A8, "uint4": UINT4}


def case_id(c):
    return "-".join(str(v).replace("torch.", "") for v in c)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def f64(t) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def adapted(name, weights, device, dtype=torch.bfloat16, seed=0):
    make, shape = LAYERS[name]
    torch.manual_seed(seed)
    layer, _ = sdnq_amd.sdnq_quantize_layer(make().to(dtype), sdnq_amd.SDNQConfig(**CFG[weights]))
    assert getattr(layer, "sdnq_dequantizer", None) is not None
    model = torch.nn.Sequential(layer.to(device))
    assert sdnq_amd.accelerate(model) == 1
    assert T.input_grad_unsupported_reason(layer, convs=True) is None
    return model, layer, shape


def randomize(layer, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.lora_up.copy_((torch.randn(layer.lora_up.shape, generator=g) * 0.05).to(layer.lora_up.device))
        layer.lora_down.copy_((torch.randn(layer.lora_down.shape, generator=g) * 0.1).to(layer.lora_down.device))


@pytest.mark.parametrize("weights", sorted(CFG))
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_zero_up_keeps_the_inference_bits(name, weights, gpu_device):
    model, layer, shape = adapted(name, weights, gpu_device)
    x = torch.randn(shape, device=gpu_device).to(torch.bfloat16)
    with torch.no_grad():
        want = [model(x).clone() for _ in range(3)][-1]
    assert sdnq_amd.add_lora(model, rank=16, seed=1, convs=True) == 1
    for _ in range(2):
        with torch.no_grad():
            y = model(x)
        assert y.grad_fn is None and y.shape == want.shape and torch.equal(bits(y), bits(want)), (name, weights, "no graph")
        y = model(x)                                                # the factors require grad
        assert y.grad_fn is not None and y.is_contiguous() and torch.equal(bits(y), bits(want)), (name, weights, "graph")
    layer.lora_down.requires_grad_(False), layer.lora_up.requires_grad_(False)
    y = model(x)                                                    # nothing requires grad: adapter inference
    assert y.grad_fn is None and torch.equal(bits(y), bits(want))
    assert sdnq_amd.remove_lora(model) == 1
    with torch.no_grad():
        assert torch.equal(bits(model(x)), bits(want))


def check(got, e, s, terms, what, extra=0.0):
    got, dt = f64(got), got.dtype
    err, lim = np.abs(got - e), L.bound(e, s, terms, dt) + extra
    worst = float((err / lim).max())
    print(what, "worst |got - e| / bound", worst, "max err", float(err.max()))
    assert got.shape == e.shape and worst <= 1.0, (what, worst, np.unravel_index(int((err / lim).argmax()), err.shape))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_outputs_and_gradients_within_the_derived_bound(case, gpu_device, monkeypatch):
    name, weights, dt, rank, route = case
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", route)
    model, layer, shape = adapted(name, weights, gpu_device, dt)
    nd = len(shape) - 2
    x = (torch.randn(shape, device=gpu_device) * 0.5).to(dt)
    layer.bias.requires_grad_()
    # the layer before the adapter goes on: its output, and QuantizedConvInputGrad's gradients on the same route
    xb = x.clone().requires_grad_()
    base = T.quantized_conv_input_grad(layer, xb)
    dy = (torch.randn(base.shape, device=gpu_device) * 0.02).to(dt)
    base.backward(dy)
    gi_base, bias_grad = xb.grad.clone(), layer.bias.grad.clone()
    layer.bias.grad = None
    alpha = 1.5 * rank
    assert sdnq_amd.add_lora(model, rank=rank, alpha=alpha, seed=1, convs=True) == 1
    randomize(layer)
    scale = float(np.float32(layer.lora_scale))
    assert layer.lora_scale == 1.5
    made = {}
    real_t, real_g = ops.conv_lowrank_down, ops.lowrank_down
    monkeypatch.setattr(lora.ops, "conv_lowrank_down", lambda *a: made.setdefault("t", real_t(*a)))
    monkeypatch.setattr(lora.ops, "lowrank_down", lambda *a: made.setdefault("g_t", real_g(*a)))
    xg = x.clone().requires_grad_()
    y = model(xg)
    y.backward(dy)
    kernel, stride, padding, dilation, _ = T._conv_geometry(layer)
    col2im = T._takes_col2im_route(1, kernel[0] * kernel[1], stride, x.numel() // shape[1])    # the base gradient's route, forced or not
    monkeypatch.undo()
    down, up = layer.lora_down.detach(), layer.lora_up.detach()
    x4, dy4 = (x.unsqueeze(2), dy.unsqueeze(2)) if nd == 1 else (x, dy)
    b, cin, h, w = x4.shape
    _, n, ho, wo = dy4.shape
    m, kprod = b * ho * wo, kernel[0] * kernel[1]
    t, g_t = made["t"][0], made["g_t"]
    assert tuple(made["t"][1]) == (b, ho, wo)
    assert torch.equal(bits(t), bits(ops.conv_lowrank_down(x4, down.reshape(rank, -1), kernel, stride, padding, dilation)[0])), "t"
    dy2d = dy4.permute(0, 2, 3, 1).reshape(m, n)
    up2d = up.reshape(n, rank)
    assert torch.equal(bits(g_t), bits(ops.lowrank_down(dy2d.contiguous(), up2d.t().contiguous()))), "g_t"
    t64, gt64, up64, dy64 = f64(t), f64(g_t), f64(up2d), f64(dy2d)
    # y = base + scale * t . up^T, NCHW
    nchw = lambda a: a.reshape(b, ho, wo, n).transpose(0, 3, 1, 2).reshape(y.shape)   # noqa: E731
    assert y.dtype == dt and y.shape == base.shape
    check(y, f64(base) + scale * nchw(t64 @ up64.T), np.abs(f64(base)) + abs(scale) * nchw(np.abs(t64) @ np.abs(up64).T), rank, (case, "y"))
    # grad_input = QuantizedConvInputGrad's + scale * conv^T(g_t, down)
    conv_t = lambda g4, d4: torch.nn.grad.conv2d_input((b, cin, h, w), d4, g4, stride=stride, padding=padding, dilation=dilation)  # noqa: E731
    g4 = g_t.double().cpu().view(b, ho, wo, rank).permute(0, 3, 1, 2).contiguous()
    d4 = down.double().cpu().reshape(rank, cin, *kernel)
    term, term_abs = conv_t(g4, d4).numpy().reshape(shape), conv_t(g4.abs(), d4.abs()).numpy().reshape(shape)
    # in place by ops.lowrank_add where its limits allow (lora._conv_adapter_grad_input); elsewhere ops.linear_float rounds the term first
    in_place = kprod * rank <= 256 and ((h * w) % 8 == 0 if col2im else cin % 8 == 0)
    assert in_place == (name != "c2d_3x3_s2" and rank == 16)                      # 9 x 9 input pixels; 9 * 32 = 288 columns
    extra = 0.0 if in_place else abs(scale) * 0.5 * L.ulp(term, dt)
    assert xg.grad.dtype == dt and xg.grad.shape == x.shape and xg.grad.is_contiguous()
    check(xg.grad, f64(gi_base) + scale * term, np.abs(f64(gi_base)) + abs(scale) * term_abs, kprod * rank, (case, "grad_input"), extra)
    # grad_up = scale * dY^T . t ; grad_down = scale * g_t^T . unfold(x)
    u64 = torch.nn.functional.unfold(x4.double().cpu(), kernel, dilation=dilation, padding=padding, stride=stride)
    u64 = u64.transpose(1, 2).reshape(m, cin * kprod).numpy()
    assert layer.lora_up.grad.shape == up.shape and layer.lora_up.grad.dtype == up.dtype
    check(layer.lora_up.grad.reshape(n, rank), scale * (dy64.T @ t64), abs(scale) * (np.abs(dy64).T @ np.abs(t64)), m, (case, "grad_up"))
    assert layer.lora_down.grad.shape == down.shape and layer.lora_down.grad.dtype == down.dtype
    check(layer.lora_down.grad.reshape(rank, -1), scale * (gt64.T @ u64), abs(scale) * (np.abs(gt64).T @ np.abs(u64)), m, (case, "grad_down"))
    assert torch.equal(bits(layer.bias.grad), bits(bias_grad)), "grad_bias"
    assert layer.weight.grad is None and layer.scale.grad is None


def test_cases_that_must_run(gpu_device):
    # an input that does not require grad: no grad_input, the factors still get theirs; float32 master factors get float32 gradients
    model, layer, shape = adapted("c2d_3x3", "w8a8", gpu_device)
    assert sdnq_amd.add_lora(model, rank=16, dtype=torch.float32, seed=4, convs=True) == 1
    randomize(layer)
    x = torch.randn(shape, device=gpu_device).to(torch.bfloat16)
    y = model(x)
    assert y.grad_fn is not None and y.dtype == torch.bfloat16
    y.float().sum().backward()
    assert x.grad is None
    assert layer.lora_up.grad.dtype == torch.float32 and layer.lora_down.grad.dtype == torch.float32
    assert layer.lora_up.grad.shape == (32, 16, 1, 1) and layer.lora_down.grad.shape == (16, 16, 3, 3)
    assert bool(layer.lora_up.grad.any()) and bool(layer.lora_down.grad.any())
    # torch.no_grad(): adapter inference, the values of the graph call
    with torch.no_grad():
        again = model(x)
    assert again.grad_fn is None and torch.equal(bits(again), bits(y))


def test_adamw_steps_on_the_adapters_lower_the_loss(gpu_device):
    torch.manual_seed(1)
    convs = [torch.nn.Conv2d(16, 32, 3, padding=1), torch.nn.Conv2d(32, 16, 3, stride=2, padding=1)]
    model = torch.nn.Sequential(*(sdnq_amd.sdnq_quantize_layer(c.to(torch.bfloat16), sdnq_amd.SDNQConfig(**W8A8))[0] for c in convs)).to(gpu_device)
    assert sdnq_amd.accelerate(model) == 2
    res = sdnq_amd.add_lora(model, rank=16, dtype=torch.float32, seed=5, convs=True)
    assert res == 2 and len(res.parameters) == 4
    opt = optim.AdamW(res.parameters, lr=2e-3, weight_decay=0.0)
    torch.manual_seed(7)
    x = torch.randn(2, 16, 12, 12, device=gpu_device).to(torch.bfloat16)
    with torch.no_grad():
        target = model(x).float() + 0.5 * torch.randn(2, 16, 6, 6, device=gpu_device)
    losses = []
    for _ in range(21):
        opt.zero_grad()
        loss = ((model(x).float() - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("losses", losses[0], losses[-1])
    assert losses[-1] < losses[0], losses
    assert all(p.grad is not None for p in res.parameters) and model[0].weight.grad is None


def test_scratch_counts_the_new_buffers_and_release_frees_them(gpu_device, monkeypatch):
    monkeypatch.delenv("SDNQ_HIP_CONV_GRAD_SLAB_MB", raising=False)
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", "gather")
    model, layer, _ = adapted("c2d_3x3", "w8a8", gpu_device)
    rank = 64
    sdnq_amd.add_lora(model, rank=rank, seed=6, convs=True)
    randomize(layer)
    T.release_scratch()
    assert T.scratch_bytes(gpu_device) == 0
    x = torch.randn(2, 16, 16, 16, device=gpu_device).to(torch.bfloat16)   # M = 512: two slabs, a workspace is needed
    model(x).float().sum().backward()                                      # the input needs no grad: no weight operand, no U_g
    workspace = 2 * 144 * rank * 4                                         # grad_down's partial sums [slab][K][rank], the larger of the two
    assert workspace > 2 * 32 * rank * 4 and T.scratch_bytes(gpu_device) == workspace
    model(x.clone().requires_grad_()).float().sum().backward()
    u_g = 512 * 9 * rank * 2                                               # [B H W][kprod rank] bf16: larger than the base gradient's U
    assert u_g > 512 * 9 * 32 * 2 and T.scratch_bytes(gpu_device) == workspace + 32 * 144 * 2 + u_g
    T.release_scratch()
    assert T.scratch_bytes(gpu_device) == 0
