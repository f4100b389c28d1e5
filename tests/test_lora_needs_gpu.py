"""Which inputs of a Linear adapter require a gradient decides what its backward launches, never what it computes (sdnq_amd/lora.py,
QuantizedLinearLoRA and QuantizedLinearDoRA through the wrappers of add_lora).

One int8 row-wise w8a8 bfloat16 Linear with a bias, K = 64, N = 48, rank 8, M = 40 rows (one partial 64-row tile of the add kernel, one
slab of the grad kernels: no workspace), as LoRA (inputs x, down, up, bias) and as DoRA (magnitude as well), with dropout off and with
dropout = 0.25 in training mode.  torch.cuda.manual_seed comes immediately before every forward, so every run draws the same
(seed, offset).  For EVERY non-empty subset of the inputs that requires a gradient -- 15 and 31, times the two dropout settings:

  * the output has the bits of the run in which all inputs require a gradient,
  * every gradient of the subset has the bits of that run's gradient (the kernels are deterministic by construction),
  * every input outside the subset ends with .grad None,
  * the library calls of the forward and of the backward are counted by pass-through wrappers and compared with the tables below, which
    follow the backward chain of the module docstring of sdnq_amd/lora.py,
  * every counted call that takes a dropout triple gets the one the forward drew.

When the bias is the only input that requires a gradient the wrapper of add_lora builds no graph (it looks at the input and the adapter's
own parameters): the output is that of the inference path, with no grad_fn.  That subset is therefore run twice: through the wrapper,
which must return the same bits without a graph, and through the autograd Function itself, whose bias gradient is compared as above.

One M = 0 call per kind, all inputs requiring a gradient: zero gradients of the parameters' shapes and dtypes, no library call in the
backward."""
import inspect
import itertools

import pytest
import torch

import sdnq_amd
from sdnq_amd import lora, ops, training
from tests.test_lora_gpu import W8A8, seeded_layer

pytestmark = pytest.mark.gpu

K, N, RANK, M = 64, 48, 8, 40
P = 0.25
SEED = 1234
INPUTS = {"lora": ("x", "down", "up", "bias"), "dora": ("x", "down", "up", "bias", "magnitude")}
COUNTED = {ops: ("lowrank_down", "lowrank_down_dropout", "lowrank_add", "lowrank_add_dropout", "lowrank_add_dora", "lowrank_grad",
                 "lowrank_grad_dropout", "dora_bwd", "dora_normsq"),
           training: ("_linear_base_grad",)}
TAKES_TRIPLE = ("lowrank_down_dropout", "lowrank_add_dropout", "lowrank_grad_dropout")

# ---- the tables: calls per forward, and calls each requested gradient adds to the backward; (dropout off, dropout on) ------------------
FORWARD = {
    "lora": ({"lowrank_down": 1, "lowrank_add": 1}, {"lowrank_down_dropout": 1, "lowrank_add": 1}),
    # the norm never sees the mask; the add with DoRA's epilogue has no dropout form (the mask is on x, in the down projection)
    "dora": ({"dora_normsq": 1, "lowrank_down": 1, "lowrank_add_dora": 1}, {"dora_normsq": 1, "lowrank_down_dropout": 1, "lowrank_add_dora": 1}),
}
BACKWARD = {
    "x": ({"_linear_base_grad": 1, "lowrank_add": 1}, {"_linear_base_grad": 1, "lowrank_add_dropout": 1}),   # grad_input = dY . W, += s g_t . down
    "down": ({"lowrank_grad": 1}, {"lowrank_grad_dropout": 1}),                                              # s g_t^T . (mask *) x
    "up": ({"lowrank_grad": 1}, {"lowrank_grad": 1}),                                                        # s dY^T . t: t is masked already
    "bias": ({}, {}),                                                                                        # dY.sum(0): torch
    "magnitude": ({}, {}),                                                                                   # q comes out of dora_bwd
}
G_T = {"lowrank_down": 1}      # g_t = dY . up, once, when x or down requires a gradient: never a dropout form (the mask is not on dY)
DORA_BACKWARD = {"dora_bwd": 1}  # g = dY * c first, on every backward with rows; want_q (and the saved y) only for the magnitude


def expected_backward(kind, subset, dropout):
    want = dict(DORA_BACKWARD) if kind == "dora" else {}
    for name in subset:
        for call, n in BACKWARD[name][dropout].items():
            want[call] = want.get(call, 0) + n
    if "x" in subset or "down" in subset:
        for call, n in G_T.items():
            want[call] = want.get(call, 0) + n
    return want


class Calls:
    """Pass-through counters on the entry points of COUNTED; the arguments of every call, bound to the parameter names."""

    def __init__(self, monkeypatch):
        self.log = []
        for module, names in COUNTED.items():
            for name in names:
                monkeypatch.setattr(module, name, self._counter(name, getattr(module, name)))

    def _counter(self, name, fn):
        sig = inspect.signature(fn)

        def counted(*args, **kwargs):
            self.log.append((name, sig.bind(*args, **kwargs).arguments))
            return fn(*args, **kwargs)
        return counted

    def take(self):
        """({name: count}, [arguments of the calls]) since the last take."""
        log, self.log = self.log, []
        counts = {}
        for name, _ in log:
            counts[name] = counts.get(name, 0) + 1
        return counts, log


def build(kind, dropout, dev):
    layer = seeded_layer(W8A8, N, K, dev)
    model = torch.nn.Sequential(layer)
    assert sdnq_amd.accelerate(model) == 1 and layer.sdnq_dequantizer.use_quantized_matmul
    res = sdnq_amd.add_lora(model, rank=RANK, alpha=12, seed=1, dropout=P if dropout else 0.0, use_dora=kind == "dora")
    assert res == 1
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        layer.lora_up.copy_((torch.randn(layer.lora_up.shape, generator=g) * 0.05).to(dev))
        layer.lora_down.copy_((torch.randn(layer.lora_down.shape, generator=g) * 0.1).to(dev))
        if kind == "dora":
            layer.lora_magnitude.mul_((1 + 0.2 * torch.randn(N, generator=g)).to(dev))
    model.train()
    torch.manual_seed(11)
    x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
    dy = (torch.randn(M, N, device=dev) * 0.02).to(torch.bfloat16)
    return model, layer, x, dy


def leaves(layer, kind, x):
    params = {"x": x, "down": layer.lora_down, "up": layer.lora_up, "bias": layer.bias}
    if kind == "dora":
        params["magnitude"] = layer.lora_magnitude
    return params


def run(model, layer, kind, x0, dy, subset, calls, through_function=False):
    """One forward + backward with exactly `subset` requiring a gradient: (y, {name: grad | None}, forward counts, backward counts, the
    logged calls, the (threshold, seed, offset) the forward must have drawn)."""
    x = x0.clone().requires_grad_("x" in subset)
    ins = leaves(layer, kind, x)
    for name, p in ins.items():
        p.requires_grad_(name in subset)
        p.grad = None
    torch.cuda.manual_seed(SEED)
    gen = torch.cuda.default_generators[x.device.index]
    drawn = (lora.dropout_threshold(P), int(gen.initial_seed()), int(gen.get_offset()))
    assert drawn[1] == SEED
    calls.take()
    if through_function:
        base = layer.forward_func._sdnq_lora_base
        if kind == "dora":
            c = lora._dora_c(layer, layer.lora_down, layer.lora_up, x.dtype)
            y = lora.QuantizedLinearDoRA.apply(layer, base, x, layer.lora_down, layer.lora_up, c, layer.bias)
        else:
            y = lora.QuantizedLinearLoRA.apply(layer, base, x, layer.lora_down, layer.lora_up, layer.bias)
    else:
        y = model(x)
    fwd, log = calls.take()
    bwd = {}
    if y.grad_fn is not None:
        y.backward(dy)
        bwd, more = calls.take()
        log += more
    return y.detach(), {name: p.grad for name, p in ins.items()}, fwd, bwd, log, drawn


def subsets(names):
    return [s for r in range(1, len(names) + 1) for s in itertools.combinations(names, r)]


@pytest.mark.parametrize("dropout", (False, True), ids=("no_dropout", "dropout"))
@pytest.mark.parametrize("kind", ("lora", "dora"))
def test_every_subset_of_required_gradients_has_the_bits_and_the_calls_of_its_table(kind, dropout, gpu_device, monkeypatch):
    model, layer, x0, dy = build(kind, dropout, gpu_device)
    calls = Calls(monkeypatch)
    names = INPUTS[kind]
    cases = subsets(names)
    assert len(cases) == {"lora": 15, "dora": 31}[kind]
    y_all, g_all, fwd_all, bwd_all, _, _ = run(model, layer, kind, x0, dy, names, calls)
    assert all(g_all[name] is not None and bool(g_all[name].any()) for name in names), "every gradient of the full run is there and nonzero"
    assert fwd_all == FORWARD[kind][dropout] and bwd_all == expected_backward(kind, names, dropout)
    for subset in cases:
        graph = any(name != "bias" for name in subset)        # the wrapper looks at the input and the adapter's own parameters
        y, grads, fwd, bwd, log, drawn = run(model, layer, kind, x0, dy, subset, calls)
        print(kind, "dropout" if dropout else "no dropout", subset, "forward", fwd, "backward", bwd)
        assert torch.equal(y, y_all), (subset, "the output bits")
        assert fwd == FORWARD[kind][dropout], (subset, "forward calls", fwd)
        if not graph:   # only the bias: the inference path, no graph -- the Function itself gives the bias its gradient
            assert bwd == {} and all(g is None for g in grads.values()), (subset, "no graph through the wrapper")
            y, grads, fwd, bwd, log, drawn = run(model, layer, kind, x0, dy, subset, calls, through_function=True)
            assert torch.equal(y, y_all), (subset, "the output bits, through the Function")
            assert fwd == FORWARD[kind][dropout], (subset, "forward calls, through the Function", fwd)
        assert bwd == expected_backward(kind, subset, dropout), (subset, "backward calls", bwd)
        for name in names:
            if name in subset:
                assert grads[name] is not None and grads[name].dtype == g_all[name].dtype, (subset, name)
                assert torch.equal(grads[name], g_all[name]), (subset, name, "the gradient bits")
            else:
                assert grads[name] is None, (subset, name, "no gradient asked for, none given")
        for name, args in log:
            if name in TAKES_TRIPLE:
                assert dropout and (args["threshold"], args["seed"], args["offset"]) == drawn, (subset, name, args, drawn)
            if name == "dora_bwd":   # the column sums q, the saved output and the workspace only where the magnitude needs them
                assert args["want_q"] == ("magnitude" in subset) and (args["y"] is not None) == ("magnitude" in subset), (subset, name)
                assert args["workspace"] is None, (subset, "one slab of rows: no workspace")
        assert dropout or not any(name in TAKES_TRIPLE for name, _ in log), (subset, "no dropout entry point with dropout off")


@pytest.mark.parametrize("kind", ("lora", "dora"))
def test_no_rows_give_zero_gradients_without_a_library_call_in_the_backward(kind, gpu_device, monkeypatch):
    model, layer, x0, dy = build(kind, False, gpu_device)
    calls = Calls(monkeypatch)
    names = INPUTS[kind]
    y, grads, _, bwd, _, _ = run(model, layer, kind, x0[:0], dy[:0], names, calls)
    assert y.shape == (0, N) and bwd == {}, bwd
    ins = leaves(layer, kind, x0[:0])
    for name in names:
        assert grads[name] is not None, name
        assert grads[name].shape == ins[name].shape and grads[name].dtype == ins[name].dtype and not grads[name].any(), name
