"""LoRA dropout through the adapter layer, end to end on the GPU (sdnq_amd/lora.py).

In train() the layer's y, grad_input, grad_down and grad_up must equal, bit for bit, the composition of the PLAIN ops calls on an input
masked on the host -- the mask the oracle predicts from the (seed, offset) read from torch's generator before the call -- with
scale_d = float32(scale 65536 / (65536 - T)): no tolerance, every step of the composition is a kernel whose bits are pinned elsewhere."""
import pytest
import torch
import torch.utils.checkpoint

import sdnq_amd
from oracle import oracle as O
from sdnq_amd import linear as LIN, lora, ops
from tests.test_lora_gpu import RANK, adapted, bits, randomize

pytestmark = pytest.mark.gpu

M = 300
LAYER_NAMES = ("int8_w8a8_n272", "uint4_g64_dequantize")   # one w8a8 int8 layer (K = 208, N = 272), one uint4 group-64 layer (K = 64, N = 72)
P = 0.1


def generator(dev):
    return torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]


def keep_mask(m, k, seed, offset, thr, dev):
    return torch.from_numpy((O.adamw_halves(m * k, seed, offset, 5) >= thr).reshape(m, k)).to(dev)


def build(name, dev, dropout, dtype=torch.bfloat16, alpha=24):
    model, layer, k, n, _, _ = adapted(name, dev, dtype)
    torch.manual_seed(11)
    x = (torch.randn(M, k, device=dev) * 0.5).to(dtype)
    dy = (torch.randn(M, n, device=dev) * 0.02).to(dtype)
    with torch.no_grad():
        base = [model(x).clone() for _ in range(3)][-1]             # (the third call runs on the layer's plan where one is built)
    assert sdnq_amd.add_lora(model, rank=RANK, alpha=alpha, seed=1, dropout=dropout) == 1
    randomize(layer)
    return model, layer, x, dy, base


def composition(layer, x, dy, base, seed, offset):
    """(y, grad_input, grad_down, grad_up) from the plain kernels on the host-masked input."""
    dev, dt = x.device, x.dtype
    thr = lora.dropout_threshold(layer.lora_dropout)
    sd = lora.dropout_scale(layer.lora_scale, thr)
    keep = keep_mask(x.shape[0], x.shape[1], seed, offset, thr, dev)
    xm = torch.where(keep, x, torch.zeros((), dtype=dt, device=dev))
    down, up = layer.lora_down.detach(), layer.lora_up.detach()
    t = ops.lowrank_down(xm, down)
    y = ops.lowrank_add(t, up, base.clone(), sd)
    g_t = ops.lowrank_down(dy, up.t().contiguous())
    dq, qw = layer.sdnq_dequantizer, LIN._state(layer).qw
    had = dq.hadamard_group_size if dq.use_hadamard else 0
    two = [torch.empty(qw.n * qw.k, device=dev, dtype=dt) for _ in range(2)]          # buffers of the test's own, not the layer's scratch
    gi = ops.linear_float(dy, ops.weight_t(qw, dt, had, two), None)
    gi = torch.where(keep, ops.lowrank_add(g_t, down.t().contiguous(), gi.clone(), sd), gi)
    return y, gi, ops.lowrank_grad(xm, g_t, sd, out_t=True), ops.lowrank_grad(dy, t, sd)


@pytest.mark.parametrize("name", LAYER_NAMES)
def test_train_mode_equals_the_plain_kernels_on_the_masked_input(name, gpu_device):
    model, layer, x, dy, base = build(name, gpu_device, P)
    model.train()
    gen = generator(gpu_device)
    torch.cuda.manual_seed(4321)
    gen.set_offset(1 << 33)                                          # an offset above 2^32
    seed, offset = gen.initial_seed(), gen.get_offset()
    assert seed == 4321 and offset == 1 << 33
    xg = x.clone().requires_grad_()
    y = model(xg)
    assert gen.get_offset() == offset + 4 and gen.initial_seed() == seed
    y.backward(dy)
    assert gen.get_offset() == offset + 4                            # the backward draws nothing
    want_y, want_gi, want_gd, want_gu = composition(layer, x, dy, base, seed, offset)
    for got, want, what in ((y, want_y, "y"), (xg.grad, want_gi, "grad_input"), (layer.lora_down.grad, want_gd, "grad_down"),
                            (layer.lora_up.grad, want_gu, "grad_up")):
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert torch.equal(bits(got), bits(want)), (name, what, int((bits(got) != bits(want)).sum()))
    assert not torch.equal(bits(y), bits(base))
    # without gradients the wrapper drops as well, as nn.Dropout does, and draws again
    with torch.no_grad():
        y2 = model(x)
    assert gen.get_offset() == offset + 8
    assert torch.equal(bits(y2), bits(composition(layer, x, dy, base, seed, offset + 4)[0]))
    assert not torch.equal(bits(y2), bits(y)), "two successive calls must use different masks"
    # the same seed and offset reproduce the run
    torch.cuda.manual_seed(4321)
    gen.set_offset(1 << 33)
    layer.lora_down.grad = layer.lora_up.grad = None
    xg2 = x.clone().requires_grad_()
    y3 = model(xg2)
    y3.backward(dy)
    assert torch.equal(bits(y3), bits(y)) and torch.equal(bits(xg2.grad), bits(xg.grad))
    assert torch.equal(bits(layer.lora_down.grad), bits(want_gd)) and torch.equal(bits(layer.lora_up.grad), bits(want_gu))


@pytest.mark.parametrize("name", LAYER_NAMES)
def test_eval_and_zero_dropout_give_the_plain_adapter_bits(name, gpu_device):
    model, layer, x, dy, base = build(name, gpu_device, P)
    twin, tl, _, _, _ = build(name, gpu_device, 0.0)
    assert tl.lora_dropout == 0.0 and torch.equal(tl.lora_down, layer.lora_down) and torch.equal(tl.lora_up, layer.lora_up)
    gen = generator(gpu_device)
    torch.cuda.manual_seed(5)
    before = gen.get_offset()

    def run(mod, lay):
        lay.lora_down.grad = lay.lora_up.grad = None
        xg = x.clone().requires_grad_()
        y = mod(xg)
        y.backward(dy)
        return y, xg.grad, lay.lora_down.grad, lay.lora_up.grad
    twin.train()
    want = run(twin, tl)                                             # dropout = 0 in train(): the adapter layer as it was
    down, up = tl.lora_down.detach(), tl.lora_up.detach()
    assert torch.equal(bits(want[0]), bits(ops.lowrank_add(ops.lowrank_down(x, down), up, base.clone(), tl.lora_scale)))
    model.eval()
    got = run(model, layer)
    for g, w, what in zip(got, want, ("y", "grad_input", "grad_down", "grad_up")):
        assert torch.equal(bits(g), bits(w)), (name, what)
    with torch.no_grad():
        assert torch.equal(bits(model(x)), bits(want[0]))
    assert gen.get_offset() == before                                # neither drew anything
    # up == 0 in train(): the adapter's sums are exactly zero, the inference call's bits stay
    model.train()
    with torch.no_grad():
        layer.lora_up.zero_()
    assert torch.equal(bits(model(x)), bits(base))
    with torch.no_grad():
        assert torch.equal(bits(model(x)), bits(base))
    assert gen.get_offset() == before + 8                            # ... though both calls drew


def test_capture_with_active_dropout_raises_and_without_it_does_not(gpu_device):
    model, layer, x, dy, base = build("int8_w8a8_n272", gpu_device, P)
    model.train()
    with torch.no_grad():
        model(x)                                                     # warm up: nothing is sized inside the capture
    torch.cuda.synchronize()
    gen = generator(gpu_device)
    before = gen.get_offset()
    with pytest.raises(RuntimeError, match="dropout"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            with torch.no_grad():
                model(x)
    torch.cuda.synchronize()
    assert gen.get_offset() == before                                # nothing was drawn
    model.eval()                                                     # eval(): captured as before
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad():
        want = model(x).clone()
        with torch.cuda.graph(graph):
            out = model(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


def test_checkpoint_replays_the_mask(gpu_device):
    model, layer, x, dy, base = build("int8_w8a8_n272", gpu_device, 0.5)
    model.train()
    gen = generator(gpu_device)

    def run(checkpointed):
        torch.cuda.manual_seed(77)
        layer.lora_down.grad = layer.lora_up.grad = None
        xg = x.clone().requires_grad_()
        y = torch.utils.checkpoint.checkpoint(model, xg, use_reentrant=False) if checkpointed else model(xg)
        y.backward(dy)
        return y.detach(), xg.grad, layer.lora_down.grad, layer.lora_up.grad, gen.get_offset()
    plain, ck = run(False), run(True)
    for a, b, what in zip(plain[:4], ck[:4], ("y", "grad_input", "grad_down", "grad_up")):
        assert torch.equal(bits(a), bits(b)), what
    assert plain[4] == ck[4] == 4                                    # the recomputation ran on the restored state and left none behind
    # the gradients are those of the mask the forward used: a recomputation under another mask would give other factor gradients
    want = composition(layer, x, dy, base, 77, 0)
    assert torch.equal(bits(ck[2]), bits(want[2])) and torch.equal(bits(ck[1]), bits(want[1]))
