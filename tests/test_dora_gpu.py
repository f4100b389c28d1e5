"""DoRA on the quantized Linear adapters, end to end on the GPU (sdnq_amd/lora.py, add_lora(use_dora=True)).

A fresh adapter (up == 0, magnitude = the kernel's own norm) has c == 1.0 exactly and returns the bits of the inference call.  With
perturbed up, down and magnitude every output is held against the float64 composition -- torch autograd on ops.dequant(...).double(),
the norm detached -- within a bound DERIVED from the roundings of the kernels' chain, never from what the kernels produce.  With
u = 2^-9 (bfloat16) or 2^-11 (float16) the unit roundoff of the layer dtype d, f = 2^-24 that of float32, and for one output element
    A = ||x_i||_2 (||Wq[n,:]||_2 + sum_r |U[n][r]| ||D[r,:]||_2) + |b[n]|   the magnitude of the base product: Cauchy-Schwarz over k, so that
                                                                           it also bounds the sum of magnitudes in a Hadamard-rotated basis;
                                                                           Wq the decoded codes, U D the layer's SVD factors (if any)
    B = |s| sum_r |up[n][r]| sum_k |down[r][k]| |x[i][k]|                  the magnitude of the adapter branch

    y           ulp_d(e) / 2                       the one rounding of the stored y
              + |c| u (2 A + B)                    the decoded weight rounded to d where the forward writes it (A), the base output z rounded
                                                   to d (|z| <= A), t rounded to d (B)
              + (K + R + 8) f ((|c| + 2) (A + B))  the K-term float32 sum of the base product, the K-term sum of t, the R-term sum of the add,
                                                   the (K + R)-term sums of normsq (a sum of squares: relative), sqrt, the division, c s,
                                                   c - 1, z - b and the two fmas -- each within f of the magnitudes it combines
    grad_input  ulp_d(e) / 2 + u (3 Ag + 2 Bg) + (N + R + 8) f (Ag + Bg)
                                                   Ag = ||g_i||_2 ||W[:,k]||_2 (+ SVD), Bg = |s| sum_r (sum_n |g| |up|) |down[r][k]|, g = dY c:
                                                   the extra rounding of g (Ag + Bg), the decoded weight (Ag), the rounded base gradient (Ag),
                                                   g_t rounded (Bg)
    grad_up     ulp(e) / 2 + 2 u S + (M + K + 8) f S,  S = |s| sum_i |g[i][n]| sum_k |down[r][k]| |x[i][k]|   (g and t rounded)
    grad_down   ulp(e) / 2 + 2 u S + (M + N + 8) f S,  S = |s| sum_i (sum_n |g| |up[n][r]|) |x[i][k]|          (g and g_t rounded)
    grad_m      [ sum_i |dY[i][n]| bound_y[i][n] + (M + 8) f sum_i |dY| |y_e - b| ] / (|c| sqrt(normsq))
              + (K + R + 8) f |e|                   q reads the SAVED y: its rounding and forward error, summed over M; then the M-term
                                                   float32 sum, the division by c and by the float32 sqrt(normsq)
    grad_bias   dY.sum(0) in the layer dtype, bit for bit (torch's own reduction)
The layers of the bound test run the float forward on the decoded weight (N % 16 == 8, or use_quantized_matmul off): a w8a8 forward
quantizes the activations, which is no rounding of the float64 composition -- such a layer is held by the bit-exact tests here (fresh
adapter, dropout composition, capture) and in tests/test_dora_exact_gpu.py."""
import numpy as np
import pytest
import torch

import sdnq_amd
from oracle import oracle as O
from sdnq_amd import linear as LIN, lora, ops, optim
from tests import lora_util as L
from tests.test_lora_gpu import W8A8, bits, f64, seeded_layer

pytestmark = pytest.mark.gpu

RANK = 16
LAYERS = {  # configuration, K, N
    "int8_n40": (W8A8, 64, 40),                                   # N % 16 == 8: the float forward on the decoded weight
    "uint4_g64": (dict(weights_dtype="uint4", group_size=64, use_quantized_matmul=False), 256, 64),
    "int8_w8a8_n64": (W8A8, 208, 64),                             # keeps the quantized matmul
    "int8_svd": (dict(**W8A8, use_svd=True, svd_rank=8), 208, 72),                       # the dense route of the norm
    "int8_hadamard": (dict(**W8A8, use_hadamard=True, hadamard_group_size=64), 64, 264),  # the dense route of the norm
}
FLOAT_FORWARD = ("int8_n40", "uint4_g64", "int8_svd", "int8_hadamard")
MS = (5, 130)


def build(name, dev, dtype=torch.bfloat16, m=130, **kw):
    cfg, k, n = LAYERS[name]
    layer = seeded_layer(cfg, n, k, dev, dtype)
    model = torch.nn.Sequential(layer)
    assert sdnq_amd.accelerate(model) == 1
    torch.manual_seed(11)
    x = (torch.randn(m, k, device=dev) * 0.5).to(dtype)
    dy = (torch.randn(m, n, device=dev) * 0.02).to(dtype)
    with torch.no_grad():
        base = [model(x).clone() for _ in range(3)][-1]             # (the third call runs on the layer's plan where one is built)
    res = sdnq_amd.add_lora(model, rank=RANK, alpha=24, seed=1, use_dora=True, **kw)
    assert res == 1 and len(res.parameters) == 3 and res.parameters[2] is layer.lora_magnitude
    return model, layer, x, dy, base


def perturb(layer, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.lora_up.copy_((torch.randn(layer.lora_up.shape, generator=g) * 0.05).to(layer.lora_up.device))
        layer.lora_down.copy_((torch.randn(layer.lora_down.shape, generator=g) * 0.1).to(layer.lora_down.device))
        layer.lora_magnitude.mul_((1 + 0.2 * torch.randn(layer.lora_magnitude.shape, generator=g)).to(layer.lora_magnitude.device))


def weight_parts(layer):
    """(W, Wq, U, D | None) in float32 on the device: the weight the forward multiplies by, the decoded codes alone, the SVD factors."""
    dq, qw = layer.sdnq_dequantizer, LIN._state(layer).qw
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    w = ops.dequant(qw, torch.float32, had)
    if not qw.desc.svd_up:
        return w, w, None, None
    return w, ops.dequant(qw, torch.float32, had, use_svd=False), qw.keep[3].float(), qw.keep[4].float()


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "f16"))
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_a_fresh_adapter_keeps_the_inference_bits_and_c_is_one(name, dtype, gpu_device):
    for m in MS:
        model, layer, x, dy, base = build(name, gpu_device, dtype, m)
        assert layer.lora_magnitude.dtype == torch.float32 and layer.lora_magnitude.shape == (LAYERS[name][2],) and layer.lora_dora is True
        c = lora._dora_c(layer, layer.lora_down, layer.lora_up, dtype)
        assert torch.equal(c.detach(), torch.ones_like(c)), "c == 1.0f exactly at initialisation"
        w = weight_parts(layer)[0]
        ref = w.double().norm(dim=1)
        assert float(((layer.lora_magnitude.detach().double() - ref).abs() / ref).max()) < (LAYERS[name][1] + 8) * 2.0 ** -24 + 2.0 ** -8
        with torch.no_grad():
            y = model(x)
        assert y.grad_fn is None and torch.equal(bits(y), bits(base)), (name, m, "no graph")
        y = model(x.clone().requires_grad_())
        assert y.grad_fn is not None and torch.equal(bits(y), bits(base)), (name, m, "graph")
        model.eval()
        with torch.no_grad():
            assert torch.equal(bits(model(x)), bits(base)), (name, m, "eval")
        assert sdnq_amd.remove_lora(model) == 1 and not hasattr(layer, "lora_magnitude") and not hasattr(layer, "lora_dora")


def check(got, e, lim, what):
    got = f64(got)
    err = np.abs(got - e)
    worst = float((err / lim).max())
    print(what, "worst |got - e| / bound", worst, "max err", float(err.max()))
    assert np.isfinite(got).all() and worst <= 1.0, (what, worst, np.unravel_index(int((err / lim).argmax()), err.shape))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", FLOAT_FORWARD)
def test_outputs_and_gradients_within_the_derived_bound(name, m, gpu_device):
    dt = torch.float16 if name == "int8_n40" and m == 130 or name == "uint4_g64" and m == 5 else torch.bfloat16
    model, layer, x, dy, _ = build(name, gpu_device, dt, m)
    perturb(layer)
    layer.bias.requires_grad_()
    k, n = LAYERS[name][1], LAYERS[name][2]
    s = float(np.float32(layer.lora_scale))
    xg = x.clone().requires_grad_()
    y = model(xg)
    y.backward(dy)
    # ---- the float64 composition: torch autograd, the norm detached ----
    w, wq, su, sd = weight_parts(layer)
    W = w.double()
    x64 = x.double().requires_grad_()
    up64, down64 = layer.lora_up.detach().double().requires_grad_(), layer.lora_down.detach().double().requires_grad_()
    m64, b64 = layer.lora_magnitude.detach().double().requires_grad_(), layer.bias.detach().double().requires_grad_()
    norm = (W + s * up64 @ down64).norm(dim=1).detach()
    c64 = m64 / norm
    y64 = c64 * (x64 @ W.T + s * (x64 @ down64.T) @ up64.T) + b64
    y64.backward(dy.double())
    # ---- the magnitudes of the bound (module docstring) ----
    u = 2.0 ** -9 if dt == torch.bfloat16 else 2.0 ** -11
    f = 2.0 ** -24
    xa, dya, upa, downa = np.abs(f64(x)), np.abs(f64(dy)), np.abs(f64(layer.lora_up)), np.abs(f64(layer.lora_down))
    ba, ca, normv = np.abs(f64(layer.bias)), np.abs(f64(c64)), f64(norm)
    rown = np.linalg.norm(f64(wq), axis=1) + (0 if su is None else np.abs(f64(su)) @ np.linalg.norm(f64(sd), axis=1))            # [N]
    coln = np.linalg.norm(f64(wq), axis=0) + (0 if su is None else np.linalg.norm(f64(su), axis=0) @ np.abs(f64(sd)))            # [K]
    A = np.linalg.norm(f64(x), axis=1)[:, None] * rown[None, :] + ba[None, :]
    tmag = xa @ downa.T                                                                                                          # [M, R]
    B = abs(s) * tmag @ upa.T
    e_y = f64(y64)
    lim_y = 0.5 * L.ulp(e_y, dt) + ca[None, :] * u * (2 * A + B) + (k + RANK + 8) * f * (ca[None, :] + 2) * (A + B)
    check(y, e_y, lim_y, (name, m, "y"))
    ga = dya * ca[None, :]
    Ag = np.linalg.norm(f64(dy) * f64(c64)[None, :], axis=1)[:, None] * coln[None, :]
    gtmag = ga @ upa                                                                                                             # [M, R]
    Bg = abs(s) * gtmag @ downa
    e_gi = f64(x64.grad)
    check(xg.grad, e_gi, 0.5 * L.ulp(e_gi, dt) + u * (3 * Ag + 2 * Bg) + (n + RANK + 8) * f * (Ag + Bg), (name, m, "grad_input"))
    e_gu, S = f64(up64.grad), abs(s) * ga.T @ tmag
    check(layer.lora_up.grad, e_gu, 0.5 * L.ulp(e_gu, dt) + 2 * u * S + (m + k + 8) * f * S, (name, m, "grad_up"))
    e_gd, S = f64(down64.grad), abs(s) * gtmag.T @ xa
    check(layer.lora_down.grad, e_gd, 0.5 * L.ulp(e_gd, dt) + 2 * u * S + (m + n + 8) * f * S, (name, m, "grad_down"))
    e_gm = f64(m64.grad)
    lim_m = ((dya * lim_y).sum(0) + (m + 8) * f * (dya * np.abs(e_y - f64(b64)[None, :])).sum(0)) / (ca * normv) + (k + RANK + 8) * f * np.abs(e_gm)
    assert layer.lora_magnitude.grad.dtype == torch.float32
    check(layer.lora_magnitude.grad, e_gm, lim_m, (name, m, "grad_m"))
    assert torch.equal(bits(layer.bias.grad), bits(dy.sum(0).to(layer.bias.dtype))), "grad_bias"
    assert layer.weight.grad is None and layer.scale.grad is None


def keep_mask(m, k, seed, offset, thr, dev):
    return torch.from_numpy((O.adamw_halves(m * k, seed, offset, 5) >= thr).reshape(m, k)).to(dev)


@pytest.mark.parametrize("name", ("int8_w8a8_n64", "uint4_g64"))
def test_dropout_equals_the_plain_dora_kernels_on_the_masked_input(name, gpu_device):
    model, layer, x, dy, base = build(name, gpu_device, m=130, dropout=0.1)
    perturb(layer)
    dev, dt = x.device, x.dtype
    down, up, mag = layer.lora_down.detach(), layer.lora_up.detach(), layer.lora_magnitude.detach()
    qw = LIN._state(layer).qw
    model.eval()
    nsq_eval = lora._layer_normsq(layer, down, up)
    model.train()
    nsq = lora._layer_normsq(layer, down, up)
    assert torch.equal(bits(nsq), bits(nsq_eval)) and torch.equal(bits(nsq), bits(ops.dora_normsq(qw, up, down, layer.lora_scale)))
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    torch.cuda.manual_seed(4321)
    gen.set_offset(1 << 33)
    seed, offset = gen.initial_seed(), gen.get_offset()
    xg = x.clone().requires_grad_()
    y = model(xg)
    assert gen.get_offset() == offset + 4
    y.backward(dy)
    # the composition of the plain DoRA kernels on the host-masked input
    thr = lora.dropout_threshold(layer.lora_dropout)
    sd = lora.dropout_scale(layer.lora_scale, thr)
    keep = keep_mask(x.shape[0], x.shape[1], seed, offset, thr, dev)
    xm = torch.where(keep, x, torch.zeros((), dtype=dt, device=dev))
    c = mag / torch.sqrt(nsq)
    b = layer.bias.detach().to(dt)
    t = ops.lowrank_down(xm, down)
    want_y = ops.lowrank_add_dora(t, up, base.clone(), sd, c, b)
    g, q = ops.dora_bwd(dy, want_y, b, c)
    g_t = ops.lowrank_down(g, up.t().contiguous())
    two = [torch.empty(qw.n * qw.k, device=dev, dtype=dt) for _ in range(2)]
    gi = ops.linear_float(g, ops.weight_t(qw, dt, 0, two), None)
    want_gi = torch.where(keep, ops.lowrank_add(g_t, down.t().contiguous(), gi.clone(), sd), gi)
    want_gd, want_gu = ops.lowrank_grad(xm, g_t, sd, out_t=True), ops.lowrank_grad(g, t, sd)
    want_gm = (q / c) / torch.sqrt(nsq)
    for got, want, what in ((y, want_y, "y"), (xg.grad, want_gi, "grad_input"), (layer.lora_down.grad, want_gd, "grad_down"),
                            (layer.lora_up.grad, want_gu, "grad_up"), (layer.lora_magnitude.grad, want_gm, "grad_m")):
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert torch.equal(bits(got), bits(want)), (name, what, int((bits(got) != bits(want)).sum()))
    assert not torch.equal(bits(y), bits(base))


def test_a_zero_magnitude_entry_and_a_frozen_magnitude(gpu_device):
    model, layer, x, dy, _ = build("int8_n40", gpu_device, m=130)
    perturb(layer)
    with torch.no_grad():
        layer.lora_magnitude[3] = 0.0
    xg = x.clone().requires_grad_()
    y = model(xg)
    y.backward(dy)
    gm = layer.lora_magnitude.grad
    assert float(gm[3]) == 0.0 and bool(torch.isfinite(gm).all()) and bool(gm.any())
    assert torch.equal(bits(y[:, 3]), bits(layer.bias.detach().to(y.dtype).expand(130, -1)[:, 3])), "c == 0: the column is the bias"
    assert all(bool(torch.isfinite(t).all()) for t in (xg.grad, layer.lora_up.grad, layer.lora_down.grad))
    want = (xg.grad.clone(), layer.lora_up.grad.clone(), layer.lora_down.grad.clone())
    # a frozen magnitude: q is skipped (ops.dora_bwd is asked for none), the other gradients keep their bits
    layer.lora_magnitude.requires_grad_(False)
    layer.lora_magnitude.grad = layer.lora_up.grad = layer.lora_down.grad = None
    asked = []
    real = ops.dora_bwd
    lora.ops.dora_bwd = lambda *a, **kw: asked.append(kw.get("want_q")) or real(*a, **kw)
    try:
        xg2 = x.clone().requires_grad_()
        model(xg2).backward(dy)
    finally:
        lora.ops.dora_bwd = real
    assert asked == [False] and layer.lora_magnitude.grad is None
    for got, w in zip((xg2.grad, layer.lora_up.grad, layer.lora_down.grad), want):
        assert torch.equal(bits(got), bits(w))


def test_one_adamw_step_moves_the_magnitude(gpu_device):
    model, layer, x, dy, _ = build("uint4_g64", gpu_device, m=130)
    perturb(layer)
    params = [layer.lora_down, layer.lora_up, layer.lora_magnitude]
    assert [p.dtype for p in params] == [torch.bfloat16, torch.bfloat16, torch.float32]       # two buckets
    opt = optim.AdamW(params, lr=1e-2, weight_decay=0.0)
    before = [p.detach().clone() for p in params]
    opt.zero_grad()
    model(x).backward(dy)
    opt.step()
    assert all(not torch.equal(bits(p), bits(b)) for p, b in zip(params, before))
    with torch.no_grad():                                           # the norm is recomputed from the moved factors: no stale cache
        c = lora._dora_c(layer, layer.lora_down, layer.lora_up, torch.bfloat16)
        nsq = ops.dora_normsq(LIN._state(layer).qw, layer.lora_up.detach(), layer.lora_down.detach(), layer.lora_scale)
    assert torch.equal(bits(c), bits(layer.lora_magnitude.detach() / torch.sqrt(nsq)))


def test_an_eval_forward_is_captured_and_replays_the_eager_bits(gpu_device):
    model, layer, x, dy, base = build("int8_w8a8_n64", gpu_device, m=130)
    perturb(layer)
    model.eval()
    with torch.no_grad():
        want = model(x).clone()                                      # warm up: nothing is sized inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with torch.cuda.graph(graph):
            out = model(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want)) and not torch.equal(bits(want), bits(base))
