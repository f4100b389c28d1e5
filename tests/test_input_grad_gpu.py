"""Input gradients through frozen quantized Linear layers on the GPU: sdnq_hip_dequant_t / sdnq_hip_transpose2d against the kernels whose
bits they must reproduce, QuantizedLinearInputGrad against a float64 product with the CPU oracle's dequantized weight, an adapter graph,
the paths that must stay what they were, and the scratch buffer.

Tolerance of every gradient check: the standing float-GEMM bound of tests/test_gpu_parity.py (assert_close_float) -- fp32 accumulation,
ONE rounding to the output dtype: max err / scale <= 2 ulp of the dtype, rel-L2 <= 2e-3 (bf16) / 5e-4 (f16) / 1e-5 (f32).  No Hadamard
doubling: the weight is un-rotated before the product."""
import numpy as np
import pytest
import torch

import sdnq_amd
from sdnq_amd import linear as L, ops, scratch, training as T
from tests.golden_util import Case, case_names
from tests.modules_util import module_from_case, to_f32_numpy
from tests.test_codebook_host import cb_case_names, load_case
from tests.test_gpu_parity import assert_close_float

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
PLAIN = [n for n in case_names() if not Case(n).has("svd_up")]
CB_PLAIN = [n for n in cb_case_names() if load_case(n)[0]["kind"] == "linear" and not load_case(n)[0]["cfg"].get("use_svd")]
SEEDED = {"uint4_g32": dict(weights_dtype="uint4", group_size=32), "int8_rowwise": dict(weights_dtype="int8", group_size=-1),
          "fp8": dict(weights_dtype="float8_e4m3fn", group_size=-1)}
SHAPES = ((40, 48), (136, 208), (72, 1040))  # a partial 64-tile on both axes; several tiles with ragged edges; many K tiles over few rows


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_dequant_t(qw, what):
    """ops.dequant_t == ops.dequant(.., use_svd=False).t() bit for bit in all three dtypes, the same bits again, nothing written behind out."""
    dev = qw.keep[0].device
    for dt in DTYPES:
        want = ops.dequant(qw, dt, 0, use_svd=False).t().contiguous()
        buf = torch.full((qw.k + 1, qw.n), 3.0, device=dev, dtype=dt)   # row K is the canary, allocated behind out
        got = ops.dequant_t(qw, dt, out=buf[:qw.k])
        assert got.shape == (qw.k, qw.n) and got.data_ptr() == buf.data_ptr()
        assert torch.equal(bits(got), bits(want)), (what, dt, int((bits(got) != bits(want)).sum()))
        assert bool((buf[qw.k] == 3.0).all()), (what, dt, "canary")
        again = ops.dequant_t(qw, dt)
        assert torch.equal(bits(again), bits(want)), (what, dt, "second call")


@pytest.mark.parametrize("name", PLAIN)
def test_dequant_t_bits_on_fixtures(name, gpu_device):
    qw = L._state(module_from_case(Case(name), gpu_device)).qw
    assert not qw.desc.svd_up
    check_dequant_t(qw, name)


@pytest.mark.parametrize("name", CB_PLAIN)
def test_dequant_t_bits_on_codebook_fixtures(name, gpu_device):
    from tests.test_codebook_gpu import fixture_layer
    meta, z = load_case(name)
    qw = L._state(fixture_layer(meta, z, gpu_device)).qw
    assert qw.desc.kind == ops._lib.KIND_CODEBOOK
    check_dequant_t(qw, name)


def seeded_layer(cfg, n, k, device, dtype=torch.bfloat16, bias=True, seed=0, **more):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=bias).to(dtype)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(**cfg, **more))
    return layer.to(device)


@pytest.mark.parametrize("nk", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", sorted(SEEDED))
def test_dequant_t_bits_on_seeded_shapes(fmt, nk, gpu_device):
    n, k = nk
    qw = L._state(seeded_layer(SEEDED[fmt], n, k, gpu_device)).qw
    assert (qw.n, qw.k) == (n, k)
    check_dequant_t(qw, (fmt, nk))


def test_dequant_t_refuses_what_it_is_not_built_for(gpu_device):
    qw = L._state(module_from_case(Case("int8_svd32_noqmm_bf16"), gpu_device)).qw
    with pytest.raises(ops._lib.SdnqHipError, match="status -5"):
        ops.dequant_t(qw, torch.bfloat16)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
@pytest.mark.parametrize("rc", ((40, 48), (136, 208)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_transpose2d(rc, dtype, gpu_device):
    r, c = rc
    g = torch.Generator().manual_seed(r * 1000 + c)
    wide = torch.randn(r, c + 24, generator=g).to(dtype).to(gpu_device)
    for x in (wide[:, :c].contiguous(), wide[:, :c], wide[:, 8:8 + c]):   # contiguous, ldx > c, ldx > c from an offset
        buf = torch.full((c + 1, r), 3.0, device=gpu_device, dtype=dtype)
        got = ops.transpose2d(x, out=buf[:c])
        assert got.shape == (c, r) and torch.equal(bits(got), bits(x.t().contiguous())), (rc, dtype, x.stride())
        assert bool((buf[c] == 3.0).all())
        assert torch.equal(bits(ops.transpose2d(x)), bits(got))


@pytest.mark.parametrize("name", case_names())
def test_grad_input_on_every_fixture(name, gpu_device):
    """Forward: the bits of the plain call.  Backward: x.grad against dY (float64) . W (float64), W the CPU oracle's dequantized weight --
    SVD product added, Hadamard rotation undone; every M of the fixture, so both sides of the 32-row rule."""
    c = Case(name)
    mod = module_from_case(c, gpu_device)
    w64 = c.oracle_module().dequantize().reshape(c.N, c.K).astype(np.float64)
    dt = mod.sdnq_dequantizer.result_dtype
    for m in c.ms():
        x = c.torch_tensor(f"x_{m}", device=gpu_device)
        with torch.no_grad():
            plain = mod(x.clone())
        xg = x.clone().requires_grad_()
        y = T.quantized_linear_input_grad(mod, xg)
        assert y.grad_fn is not None and y.dtype == plain.dtype and torch.equal(bits(y.detach()), bits(plain)), (name, m)
        g = torch.Generator().manual_seed(1000 + m)
        dy = (torch.randn(y.shape, generator=g) * 0.02).to(dt).to(gpu_device)
        y.backward(dy)
        assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == dt
        ref = dy.double().cpu().numpy().reshape(-1, c.N) @ w64
        got = to_f32_numpy(xg.grad).reshape(-1, c.K).astype(np.float64)
        scale = float(np.abs(ref).max())
        print(name, m, c.tag, "max err / scale", float(np.abs(got - ref).max()) / scale, "rel l2", float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
        assert_close_float(got, ref, c.tag, (name, m, "grad_input"))
    if mod.bias is not None:  # a bias that requires grad gets dY.sum(0); the frozen tensors get nothing
        mod.bias.requires_grad_()
        xg = x.clone().requires_grad_()
        T.quantized_linear_input_grad(mod, xg).backward(dy)
        want = dy.reshape(-1, c.N).sum(0)
        assert torch.equal(bits(mod.bias.grad), bits(want.to(mod.bias.dtype))) and mod.weight.grad is None and mod.scale.grad is None


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: TAG[d])
def test_adapter_graph_trains_through_a_quantized_layer(dtype, gpu_device):
    """x -> A (float32 Linear 64 -> K, trainable) -> cast to the layer dtype -> quantized layer -> sum(y * dY): A.weight.grad against the
    twin graph whose second layer is F.linear on ops.dequant's full weight, all in float64, within the standing bound.

    A is a float32 master adapter (what LoRA training keeps): the bound holds ONE rounding to the layer dtype, the one of grad_input.  With
    A in bfloat16 as well, torch's own GEMM rounds A.weight.grad a second time and the same check measured rel-L2 2.35e-3 against the
    bound's 2e-3 (one bfloat16 rounding alone is 1.6e-3 on every fixture of test_grad_input_on_every_fixture; 1.6e-3 * sqrt(2) = 2.3e-3)."""
    n, k, m = 144, 208, 48      # (N % 16 == 0: the layer keeps its w8a8 forward)
    q = seeded_layer(dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True), n, k, gpu_device, dtype=dtype)
    torch.manual_seed(5)
    a = torch.nn.Linear(64, k).to(gpu_device)

    class Adapted(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.q = a, q

        def forward(self, x):
            return self.q(self.a(x).to(dtype))

    model = Adapted()
    x = torch.randn(m, 64, device=gpu_device)
    dy = (torch.randn(m, n, device=gpu_device) * 0.02).to(dtype)
    assert sdnq_amd.accelerate(model) == 1
    assert model(x).grad_fn is None          # today's behaviour, and the switch is opt-in
    assert sdnq_amd.enable_input_grad(model) == 1
    y = model(x)
    assert y.grad_fn is not None and y.dtype == dtype
    (y * dy).sum().backward()
    w64 = ops.dequant(L._state(q).qw, dtype, 0).double()
    a64 = a.weight.detach().double().requires_grad_()
    h64 = torch.nn.functional.linear(x.double(), a64, a.bias.detach().double())
    (torch.nn.functional.linear(h64, w64, q.bias.detach().double()) * dy.double()).sum().backward()
    got, ref = to_f32_numpy(a.weight.grad).astype(np.float64), a64.grad.cpu().numpy()
    print("adapter", TAG[dtype], "max err / scale", float(np.abs(got - ref).max() / np.abs(ref).max()), "rel l2",
          float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
    assert_close_float(got, ref, TAG[dtype], ("A.weight.grad", TAG[dtype]))
    # five SGD steps on A lower the (linear) loss
    lr = 0.1 * float(a.weight.detach().norm() / a.weight.grad.norm())
    opt = torch.optim.SGD(a.parameters(), lr=lr)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = (model(x) * dy).float().sum()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[-1] < losses[0] and all(b < a_ for a_, b in zip(losses, losses[1:])), losses


def test_no_grad_paths_are_what_they_were(gpu_device):
    q = seeded_layer(dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True), 144, 208, gpu_device)
    model = torch.nn.Sequential(q)
    assert sdnq_amd.accelerate(model) == 1
    x = torch.randn(48, 208, device=gpu_device).to(torch.bfloat16)
    inference = q.forward_func
    before = [model(x).clone() for _ in range(3)][-1]   # (the third call runs on the layer's plan where one is built)
    assert sdnq_amd.enable_input_grad(model) == 1
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
    assert sdnq_amd.enable_input_grad(model, enabled=False) == 1 and q.forward_func is inference
    y = model(x.clone().requires_grad_())
    assert y.grad_fn is None and torch.equal(bits(y), bits(before))


def test_linked_projections_give_the_same_bits_under_grad(gpu_device):
    class Attn(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.to_q, self.to_k, self.to_v = (torch.nn.Linear(c, c, bias=True) for _ in range(3))

        def forward(self, h):
            return self.to_q(h), self.to_k(h), self.to_v(h)

    torch.manual_seed(13)
    blk = Attn(320).to(torch.bfloat16).to(gpu_device)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    for name in ("to_q", "to_k", "to_v"):
        setattr(blk, name, sdnq_amd.sdnq_quantize_layer(getattr(blk, name), cfg)[0])
    link = L.LINK_PROJECTIONS
    L.LINK_PROJECTIONS = True
    try:
        assert sdnq_amd.accelerate(blk) == 3 and "_sdnq_group" in blk.to_q.__dict__
        x = torch.randn(2, 75, 320, device=gpu_device).to(torch.bfloat16)
        with torch.no_grad():
            want = [t.clone() for t in blk(x)]
        assert sdnq_amd.enable_input_grad(blk) == 3
        xg = x.clone().requires_grad_()
        got = blk(xg)
        assert all(g.grad_fn is not None and torch.equal(bits(g.detach()), bits(w)) for g, w in zip(got, want))
        for g, w, mod in zip(got, want, (blk.to_q, blk.to_k, blk.to_v)):   # dY = 2 y, exact in bfloat16
            gi, = torch.autograd.grad((g.float() ** 2).sum(), xg, retain_graph=True)
            ref = (2 * w).double().reshape(-1, 320) @ ops.dequant(L._state(mod).qw, torch.bfloat16, 0).double()
            assert_close_float(to_f32_numpy(gi).reshape(-1, 320).astype(np.float64), ref.cpu().numpy(), "bf16", "linked grad_input")
        with torch.no_grad():
            again = blk(x)
        assert all(torch.equal(bits(a), bits(w)) for a, w in zip(again, want))
    finally:
        L.LINK_PROJECTIONS = link


def test_scratch_is_one_buffer_of_the_largest_layer(gpu_device):
    cfg = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    sizes = ((208, 64), (336, 208), (136, 336))       # (N, K): N * K = 13312, 69888, 45696
    layers = [seeded_layer(cfg, n, k, gpu_device, seed=i) for i, (n, k) in enumerate(sizes)]
    model = torch.nn.Sequential(*layers)
    assert sdnq_amd.accelerate(model) == 3 and sdnq_amd.enable_input_grad(model) == 3
    x = torch.randn(48, 64, device=gpu_device).to(torch.bfloat16)
    for _ in range(4):                                   # kernel-ready state, plans and workspaces exist before anything is measured
        model(x.clone().requires_grad_()).float().sum().backward()
        L.clear_activation_cache()
    T.release_scratch()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu_device)
    xg = x.clone().requires_grad_()
    model(xg).float().sum().backward()
    L.clear_activation_cache()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated(gpu_device)
    largest = max(n * k for n, k in sizes) * 2
    print("scratch", T.scratch_bytes(gpu_device), "allocated", after - before)
    assert T.scratch_bytes(gpu_device) == largest and "decoded" not in scratch.held(gpu_device)
    grads = 2 * xg.numel() * 2                            # xg and xg.grad
    assert after - before <= largest + grads + 3 * 512, (after - before, largest, grads)   # (the allocator rounds a block up to 512 bytes)
    # a Hadamard layer brings the second buffer, of the same size
    had = seeded_layer(dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, use_hadamard=True, hadamard_group_size=64), 72, 128,
                       gpu_device)
    assert had.sdnq_dequantizer.use_hadamard
    hx = torch.randn(48, 128, device=gpu_device).to(torch.bfloat16).requires_grad_()
    T.quantized_linear_input_grad(had, hx).float().sum().backward()
    assert T.scratch_bytes(gpu_device) == 2 * largest
    first = scratch.held(gpu_device)["operand"].data_ptr()
    model(x.clone().requires_grad_()).float().sum().backward()
    assert T.scratch_bytes(gpu_device) == 2 * largest and scratch.held(gpu_device)["operand"].data_ptr() == first   # reused, not regrown
    T.release_scratch()
