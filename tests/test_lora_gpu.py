"""Trainable low-rank adapters on frozen quantized Linear layers, end to end on the GPU (sdnq_amd/lora.py).

With up = 0 the adapter changes no bit of the layer's output, with and without a graph.  With random factors the outputs cannot be
bit-exact against a CPU composition -- t and g_t are rounded to the layer dtype between the two products -- so each is held to a DERIVED
bound on the kernel's own t and g_t (which are compared with ops.lowrank_down bit for bit): with e the float64 composition of the same
steps, an output that reduces over L terms and is stored in dtype d satisfies

    |got - e| <= ulp_d(e) / 2 + (L + 2) 2^-24 S            S = the sum of the magnitudes of the terms, base value included

-- one rounding to d of a float32 value whose L additions, scale and base-value addition each err by at most 2^-24 of S
(tests/lora_util.bound).  y and grad_input have L = rank (the base value of grad_input is ops.linear_float's own rounded output),
grad_up and grad_down L = M."""
import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import linear as LIN, lora, ops, optim, training as T
from tests import lora_util as L

pytestmark = pytest.mark.gpu

RANK = 16
W8A8 = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
LAYERS = {  # configuration, K, N
    "int8_w8a8": (W8A8, 208, 264),          # (N % 16 == 8: the quantizer switches such a layer to the dequantize mode, int8 row-wise all the same)
    # N % 16 == 0: these keep the quantized matmul forward (asserted in adapted())
    "int8_w8a8_n272": (W8A8, 208, 272),
    "int8_svd_n80": (dict(**W8A8, use_svd=True, svd_rank=8), 208, 80),
    "int8_hadamard_n272": (dict(**W8A8, use_hadamard=True, hadamard_group_size=64), 64, 272),
    "uint4_g64_dequantize": (dict(weights_dtype="uint4", group_size=64, use_quantized_matmul=False), 64, 72),
    "int8_svd": (dict(**W8A8, use_svd=True, svd_rank=8), 208, 72),
    "int8_hadamard": (dict(**W8A8, use_hadamard=True, hadamard_group_size=64), 64, 264),
}
MS = (40, 300)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def f64(t) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def seeded_layer(cfg, n, k, device, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=True).to(dtype)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(**cfg))
    return layer.to(device)


def adapted(name, device, dtype=torch.bfloat16, factor_dtype=None, alpha=24):
    cfg, k, n = LAYERS[name]
    layer = seeded_layer(cfg, n, k, device, dtype)
    model = torch.nn.Sequential(layer)
    assert sdnq_amd.accelerate(model) == 1
    assert bool(layer.sdnq_dequantizer.use_quantized_matmul) == bool(cfg["use_quantized_matmul"] and n % 16 == 0)
    return model, layer, k, n, factor_dtype, alpha


def randomize(layer, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.lora_up.copy_((torch.randn(layer.lora_up.shape, generator=g) * 0.05).to(layer.lora_up.device))
        layer.lora_down.copy_((torch.randn(layer.lora_down.shape, generator=g) * 0.1).to(layer.lora_down.device))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_zero_up_keeps_the_inference_bits(name, m, gpu_device):
    model, layer, k, n, _, _ = adapted(name, gpu_device)
    x = torch.randn(2, m // 2, k, device=gpu_device).to(torch.bfloat16)
    with torch.no_grad():
        want = [model(x).clone() for _ in range(3)][-1]            # (the third call runs on the layer's plan where one is built)
    assert sdnq_amd.add_lora(model, rank=RANK, seed=1) == 1
    for _ in range(2):
        with torch.no_grad():
            y = model(x)
        assert y.grad_fn is None and y.shape == want.shape and torch.equal(bits(y), bits(want)), (name, m, "no graph")
        y = model(x)                                                # the factors require grad
        assert y.grad_fn is not None and torch.equal(bits(y), bits(want)), (name, m, "graph")
    layer.lora_down.requires_grad_(False), layer.lora_up.requires_grad_(False)
    y = model(x)                                                    # nothing requires grad: adapter inference
    assert y.grad_fn is None and torch.equal(bits(y), bits(want))
    assert sdnq_amd.remove_lora(model) == 1
    with torch.no_grad():
        assert torch.equal(bits(model(x)), bits(want))


def check(got, e, s, terms, what):
    got, dt = f64(got), got.dtype
    err, lim = np.abs(got - e), L.bound(e, s, terms, dt)
    worst = float((err / lim).max())
    print(what, "worst |got - e| / bound", worst, "max err", float(err.max()))
    assert worst <= 1.0, (what, worst, np.unravel_index(int((err / lim).argmax()), err.shape))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_outputs_and_gradients_within_the_derived_bound(name, m, gpu_device, monkeypatch):
    dt = torch.float16 if name == "int8_w8a8" and m == 40 else torch.bfloat16   # one float16 layer
    model, layer, k, n, _, alpha = adapted(name, gpu_device, dt)
    x = (torch.randn(m, k, device=gpu_device) * 0.5).to(dt)
    dy = (torch.randn(m, n, device=gpu_device) * 0.02).to(dt)
    with torch.no_grad():
        base = model(x).clone()
    assert sdnq_amd.add_lora(model, rank=RANK, alpha=alpha, seed=1) == 1
    randomize(layer)
    layer.bias.requires_grad_()
    scale = float(np.float32(layer.lora_scale))
    assert layer.lora_scale == alpha / RANK
    made = []
    real = ops.lowrank_down
    monkeypatch.setattr(lora.ops, "lowrank_down", lambda *a: made.append(real(*a)) or made[-1])
    xg = x.clone().requires_grad_()
    y = model(xg)
    y.backward(dy)
    monkeypatch.undo()
    down, up = layer.lora_down.detach(), layer.lora_up.detach()
    t, g_t = made
    assert torch.equal(bits(t), bits(ops.lowrank_down(x, down))), "t"
    assert torch.equal(bits(g_t), bits(ops.lowrank_down(dy, up.t().contiguous()))), "g_t"
    t64, gt64, up64, down64, x64, dy64 = f64(t), f64(g_t), f64(up), f64(down), f64(x), f64(dy)
    # y = base + scale * t . up^T
    check(y, f64(base) + scale * (t64 @ up64.T), np.abs(f64(base)) + abs(scale) * (np.abs(t64) @ np.abs(up64).T), RANK, (name, m, "y"))
    # grad_input = linear_float(dY, W^T) + scale * g_t . down
    dq, qw = layer.sdnq_dequantizer, LIN._state(layer).qw
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    two = [torch.empty(qw.n * qw.k, device=gpu_device, dtype=dt) for _ in range(2)]   # buffers of the test's own, not the layer's scratch
    gi_base = ops.linear_float(dy, ops.weight_t(qw, dt, had, two), None)
    assert xg.grad.dtype == dt and xg.grad.shape == x.shape
    check(xg.grad, f64(gi_base) + scale * (gt64 @ down64), np.abs(f64(gi_base)) + abs(scale) * (np.abs(gt64) @ np.abs(down64)), RANK,
          (name, m, "grad_input"))
    # grad_up = scale * dY^T . t ; grad_down = scale * g_t^T . x
    assert layer.lora_up.grad.shape == up.shape and layer.lora_up.grad.dtype == up.dtype
    check(layer.lora_up.grad, scale * (dy64.T @ t64), abs(scale) * (np.abs(dy64).T @ np.abs(t64)), m, (name, m, "grad_up"))
    assert layer.lora_down.grad.shape == down.shape and layer.lora_down.grad.dtype == down.dtype
    check(layer.lora_down.grad, scale * (gt64.T @ x64), abs(scale) * (np.abs(gt64).T @ np.abs(x64)), m, (name, m, "grad_down"))
    assert torch.equal(bits(layer.bias.grad), bits(dy.sum(0).to(layer.bias.dtype))), "grad_bias"
    assert layer.weight.grad is None and layer.scale.grad is None


def test_linked_projections_keep_their_bits_and_train(gpu_device):
    class Attn(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.to_q, self.to_k, self.to_v = (torch.nn.Linear(c, c, bias=True) for _ in range(3))

        def forward(self, h):
            return self.to_q(h), self.to_k(h), self.to_v(h)

    torch.manual_seed(13)
    blk = Attn(320).to(torch.bfloat16).to(gpu_device)
    cfg = sdnq_amd.SDNQConfig(**W8A8)
    for name in ("to_q", "to_k", "to_v"):
        setattr(blk, name, sdnq_amd.sdnq_quantize_layer(getattr(blk, name), cfg)[0])
    link = LIN.LINK_PROJECTIONS
    LIN.LINK_PROJECTIONS = True
    try:
        assert sdnq_amd.accelerate(blk) == 3 and "_sdnq_group" in blk.to_q.__dict__
        x = torch.randn(2, 75, 320, device=gpu_device).to(torch.bfloat16)
        with torch.no_grad():
            want = [t.clone() for t in blk(x)]
        assert sdnq_amd.add_lora(blk, rank=RANK, seed=2) == 3
        with torch.no_grad():
            got = blk(x)
        assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want)), "no graph"
        xg = x.clone().requires_grad_()
        got = blk(xg)
        assert all(g.grad_fn is not None and torch.equal(bits(g), bits(w)) for g, w in zip(got, want)), "graph"
        sum((g.float() ** 2).sum() for g in got).backward()
        assert xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all())
        # up == 0: every grad_down is exactly zero, every grad_up is not
        for mod in (blk.to_q, blk.to_k, blk.to_v):
            assert not mod.lora_down.grad.any() and bool(mod.lora_up.grad.any())
        # with an adapter that is not zero the linked outputs differ from the inference bits, each member by its own factors
        for i, mod in enumerate((blk.to_q, blk.to_k, blk.to_v)):
            randomize(mod, seed=20 + i)
        with torch.no_grad():
            got = blk(x)
            for g, w, mod in zip(got, want, (blk.to_q, blk.to_k, blk.to_v)):
                t = ops.lowrank_down(x.reshape(-1, 320), mod.lora_down.detach())
                e = f64(w).reshape(-1, 320) + f64(t) @ f64(mod.lora_up).T
                s = np.abs(f64(w)).reshape(-1, 320) + np.abs(f64(t)) @ np.abs(f64(mod.lora_up)).T
                check(g.reshape(-1, 320), e, s, RANK, "linked y")
    finally:
        LIN.LINK_PROJECTIONS = link


def test_a_compiled_model_runs_the_adapter_as_the_whole_layer_operator(gpu_device):
    """torch.compile of the wrapper is out of scope, but a compiled model must not drop the adapter: the layer traces as the opaque
    sdnq_hip::layer_forward operator, which calls the wrapper -- the bits of eager adapter inference -- also after the plan was derived again."""
    model, layer, k, n, _, _ = adapted("int8_w8a8_n272", gpu_device)
    assert layer.__dict__["_sdnq_hip_plan"] is not None                      # without an adapter: rowquant + matmul operators
    assert sdnq_amd.add_lora(model, rank=RANK, seed=8) == 1
    randomize(layer)
    from sdnq_amd import torch_ops
    torch_ops.layer_handle(layer)                                           # whoever derives the layer's compile plan again finds none
    assert layer.__dict__["_sdnq_hip_plan"] is None and layer.forward_func.__module__ == "sdnq_amd.lora"
    x = torch.randn(40, k, device=gpu_device).to(torch.bfloat16)
    with torch.no_grad():
        eager = model(x).clone()
        compiled = torch.compile(model, fullgraph=True)(x)
    assert torch.equal(bits(compiled), bits(eager))
    sdnq_amd.remove_lora(model)
    with torch.no_grad():
        assert not torch.equal(bits(model(x)), bits(eager))                # the adapter did change the output
    assert layer.__dict__["_sdnq_hip_plan"] is not None


def test_cases_that_must_run(gpu_device):
    # an input that does not require grad: no grad_input, the factors still get theirs; float32 master factors get float32 gradients
    model, layer, k, n, _, _ = adapted("int8_w8a8", gpu_device)
    assert sdnq_amd.add_lora(model, rank=RANK, dtype=torch.float32, seed=4) == 1
    randomize(layer)
    x = torch.randn(40, k, device=gpu_device).to(torch.bfloat16)
    y = model(x)
    assert y.grad_fn is not None and y.dtype == torch.bfloat16
    y.float().sum().backward()
    assert x.grad is None
    assert layer.lora_up.grad.dtype == torch.float32 and layer.lora_down.grad.dtype == torch.float32
    assert bool(layer.lora_up.grad.any()) and bool(layer.lora_down.grad.any())
    # the same gradients as bfloat16 factors holding the same values would get, before their rounding
    up_grad32 = layer.lora_up.grad.clone()
    twin, tl, _, _, _, _ = adapted("int8_w8a8", gpu_device)
    sdnq_amd.add_lora(twin, rank=RANK, seed=4)
    with torch.no_grad():
        tl.lora_up.copy_(layer.lora_up), tl.lora_down.copy_(layer.lora_down)
        layer.lora_up.copy_(tl.lora_up), layer.lora_down.copy_(tl.lora_down)   # the float32 masters hold bfloat16 values from here on
    layer.lora_up.grad = layer.lora_down.grad = None
    model(x).float().sum().backward()
    twin(x).float().sum().backward()
    assert torch.equal(bits(layer.lora_up.grad.to(torch.bfloat16)), bits(tl.lora_up.grad))
    assert torch.equal(bits(layer.lora_down.grad.to(torch.bfloat16)), bits(tl.lora_down.grad))
    assert up_grad32.shape == tl.lora_up.grad.shape
    # M = 0
    x0 = torch.zeros(0, k, device=gpu_device, dtype=torch.bfloat16, requires_grad=True)
    layer.lora_up.grad = layer.lora_down.grad = None
    y0 = model(x0)
    assert y0.shape == (0, n)
    y0.sum().backward()
    assert x0.grad.shape == (0, k) and not layer.lora_up.grad.any() and not layer.lora_down.grad.any()
    with torch.no_grad():
        assert model(x0).shape == (0, n)


def test_adamw_steps_on_the_adapters_lower_the_loss(gpu_device):
    cfg = W8A8
    layers = [seeded_layer(cfg, 208, 64, gpu_device, seed=1), seeded_layer(cfg, 72, 208, gpu_device, seed=2)]
    model = torch.nn.Sequential(*layers)
    assert sdnq_amd.accelerate(model) == 2
    res = sdnq_amd.add_lora(model, rank=RANK, dtype=torch.float32, seed=5)
    assert res == 2 and len(res.parameters) == 4
    opt = optim.AdamW(res.parameters, lr=2e-3, weight_decay=0.0)
    torch.manual_seed(7)
    x = torch.randn(300, 64, device=gpu_device).to(torch.bfloat16)
    with torch.no_grad():
        target = model(x).float() + 0.5 * torch.randn(300, 72, device=gpu_device)
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


def test_scratch_counts_the_workspace_and_release_frees_it(gpu_device):
    model, layer, k, n, _, _ = adapted("int8_w8a8", gpu_device)
    sdnq_amd.add_lora(model, rank=RANK, seed=6)
    T.release_scratch()
    assert T.scratch_bytes(gpu_device) == 0
    x = torch.randn(300, k, device=gpu_device).to(torch.bfloat16)          # two slabs: a workspace is needed
    model(x).float().sum().backward()                                      # the input needs no grad: no weight operand
    slabs = -(-300 // L.LRG_SLAB)
    assert T.scratch_bytes(gpu_device) == slabs * n * RANK * 4             # grad_up's partial sums, the larger of the two (N > K)
    model(x.clone().requires_grad_()).float().sum().backward()
    assert T.scratch_bytes(gpu_device) == slabs * n * RANK * 4 + n * k * 2  # ... plus the transposed weight of grad_input
    T.release_scratch()
    assert T.scratch_bytes(gpu_device) == 0
    model(x[:40]).float().sum().backward()                                 # one slab: none
    assert T.scratch_bytes(gpu_device) == 0
