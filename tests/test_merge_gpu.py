"""Merging adapters into the stored codes, end to end on the GPU (sdnq_amd/lora.py: merge_lora, merge_lora_state_dict, _merge_layer).

(a) The error bound, on random data.  With W the float32 value of the stored codes (ops.dequant without SVD factors and without undoing
the rotation), E = W + s up down in float64, D = ops.dequant of the merged tensors and s'[n][g] the merged scale, EVERY element satisfies

    |D - E| <= 0.5 s'[n][g] + eps,    eps = (R + 2) f a + 4 f (qmax - qmin + 2) s'[n][g] + 2 f |D|,    f = 2^-24

derived from the roundings, never from what the kernel gives:
    (R + 2) f a     a = |W| + |s| sum_r |up| |down|: the R-term float32 sum of the rank product (its products are exact: 16-bit operands)
                    and the one rounding of e = fma(s, acc, W)
    the quantizer   q = fl((e - zp) / s') carries one rounding of e - zp (|e - zp| <= (qmax - qmin) s' (1 + f)) and one of the quotient
                    (|q| <= qmax - qmin + 1), s' itself is one rounding of (max - min) / (qmax - qmin) or amax / qmax, and the clamp cuts
                    what those roundings push past the ends: together below 4 f (qmax - qmin + 2) s' in units of the weight; the rounding to
                    the nearest code is the 0.5 s'
    2 f |D|         the dequantizer's one rounding of code * s' (+ zp, an fma), and zp = min's own
A Hadamard layer stores the rotated weight and the kernel reads dr = round_d(ops.hadamard(down)) while E holds the exact rotation
down H: eps gains |s| sum_r |up[n][r]| (u_d + g f) (|down| |H|)[r][k] -- the rounding of dr to the layer dtype (u_d = 2^-9 bfloat16,
2^-12 float16, of a magnitude below |down| |H|) and the g-term float32 sum behind it.  A DoRA merge multiplies by c = m / sqrt(normsq):
eps gains (K + R + 10) f |E| for the float32 norm (a (K + R)-term sum of squares), its sqrt, the division and the multiply (the terms
tests/test_dora_gpu.py derives).  No element is exempt.  Measured worst |D - E| / bound: README.md.

(b) A toy model with linked to_q / to_k / to_v and a plain layer; (c) the composition route on exact-sum operands."""
import copy

import numpy as np
import pytest
import torch

import sdnq_amd
from oracle import oracle as O
from sdnq_amd import linear as LIN, lora, ops
from sdnq_amd.common import dtype_dict
from tests import dora_util as D
from tests.golden_util import Case
from tests.modules_util import module_from_case
from tests.test_lora_gpu import W8A8, bits, f64, seeded_layer

pytestmark = pytest.mark.gpu
F = 2.0 ** -24
U4G64 = dict(weights_dtype="uint4", group_size=64, use_quantized_matmul=False)
CASES = {  # name -> (layer factory, rank)
    "int8_rowwise": (lambda dev: seeded_layer(W8A8, 72, 208, dev), 16),
    "uint4_g64": (lambda dev: seeded_layer(U4G64, 72, 320, dev, torch.float16), 24),
    "int5_g16": (lambda dev: seeded_layer(dict(weights_dtype="int5", group_size=16, use_quantized_matmul=False), 40, 272, dev), 8),
    "fixture_int8_svd32": (lambda dev: module_from_case(Case("int8_svd32_noqmm_bf16"), dev), 16),
    "fixture_int8_had64": (lambda dev: module_from_case(Case("int8_had64_k192_qmm_bf16"), dev), 16),
}


def stored(layer):
    """(W float64 [N, K], scale float64 [N, K] spread over the groups, qw) of the layer's stored codes."""
    qw = LIN._state(layer).qw
    w = f64(ops.dequant(qw, torch.float32, 0, use_svd=False))
    s = f64(layer.scale.float()).reshape(qw.n, -1)
    return w, np.repeat(s, qw.k // s.shape[1], axis=1), qw


def bound(layer, e, a, d, sk, rank):
    ent = dtype_dict[layer.sdnq_dequantizer.weights_dtype]
    return 0.5 * sk + (rank + 2) * F * a + 4 * F * (ent["max"] - ent["min"] + 2) * sk + 2 * F * np.abs(d)


def check(d, e, lim, what):
    err = np.abs(d - e)
    worst = float((err / lim).max())
    print(what, "worst |D - E| / bound", round(worst, 4), "max err", float(err.max()))
    assert np.isfinite(d).all() and worst <= 1.0, (what, worst, np.unravel_index(int((err / lim).argmax()), err.shape))


def factors(n, k, rank, dt, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    up = (torch.randn((n, rank), generator=g) * 0.05).to(dt).to(dev)
    down = (torch.randn((rank, k), generator=g) * 0.1).to(dt).to(dev)
    return up, down


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_element_within_half_a_step_of_the_merged_scale(name, gpu_device):
    make, rank = CASES[name]
    layer = make(gpu_device)
    dq = layer.sdnq_dequantizer
    dt, s = dq.result_dtype, 1.5
    w, _, qw = stored(layer)
    up, down = factors(qw.n, qw.k, rank, dt, gpu_device)
    old = {n: getattr(layer, n) for n in ("weight", "scale", "zero_point", "svd_up", "svd_down", "bias")}
    d64, extra = f64(down), 0.0
    if dq.use_hadamard:
        g = dq.hadamard_group_size
        h = np.kron(np.eye(qw.k // g), O.hadamard_matrix(g, "bf16" if dt == torch.bfloat16 else "f16").astype(np.float64))
        u_d = 2.0 ** -9 if dt == torch.bfloat16 else 2.0 ** -12
        extra = abs(s) * np.abs(f64(up)) @ ((u_d + g * F) * (np.abs(d64) @ np.abs(h)))
        d64 = d64 @ h
    e = w + s * f64(up) @ d64
    a = np.abs(w) + abs(s) * np.abs(f64(up)) @ np.abs(d64)
    route = lora._merge_layer(layer, down, up, s, None)
    assert route == "fused", name
    for n, t in old.items():  # new parameter objects of the old form; factors and bias untouched
        new = getattr(layer, n)
        if n in ("svd_up", "svd_down", "bias") or t is None:
            assert new is t, n
        else:
            assert new is not t and new.shape == t.shape and new.stride() == t.stride() and new.dtype == t.dtype and not new.requires_grad, n
    d, sk, _ = stored(layer)
    check(d, e, bound(layer, e, a, d, sk, rank) + extra, name)


def test_a_dora_layer_merges_with_c_applied(gpu_device):
    layer = seeded_layer(W8A8, 72, 208, gpu_device)
    model = torch.nn.Sequential(layer)
    assert sdnq_amd.accelerate(model) == 1 and sdnq_amd.add_lora(model, rank=16, alpha=24, seed=1, use_dora=True) == 1
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        layer.lora_up.copy_((torch.randn(layer.lora_up.shape, generator=g) * 0.05).to(gpu_device))
        layer.lora_magnitude.mul_((1 + 0.2 * torch.randn(layer.lora_magnitude.shape, generator=g)).to(gpu_device))
    w, _, qw = stored(layer)
    up, down, m, s = f64(layer.lora_up), f64(layer.lora_down), f64(layer.lora_magnitude), layer.lora_scale
    inner = w + s * up @ down
    c = m / np.sqrt((inner * inner).sum(1))
    e = c[:, None] * inner
    a = np.abs(c)[:, None] * (np.abs(w) + abs(s) * np.abs(up) @ np.abs(down))
    res = sdnq_amd.merge_lora(model)
    assert res == 1 and res.merged == ["0"] and res.skipped == [] and not hasattr(layer, "lora_magnitude")
    assert layer.forward_func.__module__ != "sdnq_amd.lora"
    d, sk, _ = stored(layer)
    check(d, e, bound(layer, e, a, d, sk, 16) + (qw.k + 16 + 10) * F * np.abs(e), "DoRA int8 row-wise")


class Toy(torch.nn.Module):
    def __init__(self, c=320):
        super().__init__()
        self.to_q, self.to_k, self.to_v = (torch.nn.Linear(c, c, bias=True) for _ in range(3))
        self.proj = torch.nn.Linear(c, 72, bias=True)

    def forward(self, h):
        return self.to_q(h), self.to_k(h), self.to_v(h), self.proj(h)


NAMES = ("to_q", "to_k", "to_v", "proj")
FIELDS = ("weight", "scale", "zero_point")


def toy(dev, accelerate=True):
    torch.manual_seed(13)
    blk = Toy().to(torch.bfloat16)
    cfg = sdnq_amd.SDNQConfig(**W8A8)
    for name in NAMES:
        setattr(blk, name, sdnq_amd.sdnq_quantize_layer(getattr(blk, name), cfg)[0])
    blk = blk.to(dev)
    if accelerate:
        assert sdnq_amd.accelerate(blk) == 4 and "_sdnq_group" in blk.to_q.__dict__
    return blk, cfg


def randomize(blk, seed=20):
    for i, name in enumerate(NAMES):
        mod = getattr(blk, name)
        g = torch.Generator().manual_seed(seed + i)
        with torch.no_grad():
            mod.lora_up.copy_((torch.randn(mod.lora_up.shape, generator=g) * 0.05).to(mod.lora_up.device))
            mod.lora_down.copy_((torch.randn(mod.lora_down.shape, generator=g) * 0.1).to(mod.lora_down.device))


def run(blk, x):
    with torch.no_grad():
        return [[t.clone() for t in blk(x)] for _ in range(3)][-1]  # (the third call runs on the plans where they are built)


def same_tensors(a, b):
    for name in NAMES:
        for f in FIELDS:
            ta, tb = getattr(getattr(a, name), f), getattr(getattr(b, name), f)
            assert (ta is None) == (tb is None), (name, f)
            if ta is not None:
                assert ta.dtype == tb.dtype and ta.shape == tb.shape, (name, f)
                assert torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8)), (name, f)


@pytest.mark.parametrize("plans", (True, False), ids=("plans", "no plans"))
def test_a_merged_model_runs_as_a_fresh_model_of_the_merged_tensors(plans, gpu_device, monkeypatch, tmp_path):
    monkeypatch.setattr(LIN, "LINK_PROJECTIONS", True)
    if not plans:
        monkeypatch.setattr(LIN, "FAST_PLANS", False)
    blk, cfg = toy(gpu_device)
    x = torch.randn(2, 75, 320, device=gpu_device).to(torch.bfloat16)
    base = run(blk, x)
    assert sdnq_amd.add_lora(blk, rank=8, seed=2) == 4
    randomize(blk)
    adapted = run(blk, x)
    old = {n: getattr(blk, n).weight for n in NAMES}
    res = sdnq_amd.merge_lora(blk)
    assert res == 4 and res.merged == list(NAMES) and res.skipped == []
    assert all(getattr(blk, n).weight is not old[n] and not hasattr(getattr(blk, n), "lora_down") for n in NAMES)
    got = run(blk, x)
    assert all(not torch.equal(bits(g), bits(b)) for g, b in zip(got, base)), "the merged weights are in use"
    # the adapter's effect is there: closer to the adapted output than the base output is
    for g, b, a in zip(got, base, adapted):
        assert float((g.float() - a.float()).abs().mean()) < 0.5 * float((b.float() - a.float()).abs().mean())
    fresh, _ = toy(gpu_device, accelerate=False)
    for name in NAMES:
        for f in FIELDS:
            t = getattr(getattr(blk, name), f)
            if t is not None:
                setattr(getattr(fresh, name), f, torch.nn.Parameter(t.detach().clone(), requires_grad=False))
                assert getattr(getattr(fresh, name), f).stride() == t.stride()
    assert sdnq_amd.accelerate(fresh) == 4 and "_sdnq_group" in fresh.to_q.__dict__
    want = run(fresh, x)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want)), "eager output of the merged model != a fresh model's"
    # a plain quantized checkpoint: the merged tensors round-trip through save_sdnq_model / load_sdnq_model
    sdnq_amd.save_sdnq_model(blk, str(tmp_path), sdnq_config=cfg)
    with torch.device("meta"):
        skeleton = Toy().to(torch.bfloat16)
    loaded = sdnq_amd.load_sdnq_model(str(tmp_path), model=skeleton, device=gpu_device)
    same_tensors(blk, loaded)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(run(loaded, x), got))


def test_a_rank_4_file_equals_the_zero_padded_adapter(gpu_device, monkeypatch):
    monkeypatch.setattr(LIN, "LINK_PROJECTIONS", True)
    a_model, _ = toy(gpu_device)
    b_model, _ = toy(gpu_device)
    g = torch.Generator().manual_seed(7)
    sd = {}
    for name in NAMES:
        n = getattr(a_model, name).sdnq_dequantizer.out_features
        sd[f"base_model.model.{name}.lora_A.default.weight"] = torch.randn((4, 320), generator=g) * 0.1
        sd[f"base_model.model.{name}.lora_B.default.weight"] = torch.randn((n, 4), generator=g) * 0.05
    res = sdnq_amd.merge_lora_state_dict(a_model, sd, scale=2.0)
    assert res == 4 and res.merged == list(NAMES)
    assert sdnq_amd.add_lora(b_model, rank=8, alpha=16, seed=1) == 4       # scale = alpha / rank = 2
    padded = {}
    for name in NAMES:
        down, up = lora.pad_rank(sd[f"base_model.model.{name}.lora_A.default.weight"], sd[f"base_model.model.{name}.lora_B.default.weight"])
        padded[f"{name}.lora_A.weight"], padded[f"{name}.lora_B.weight"] = down, up
    assert sdnq_amd.load_lora_state_dict(b_model, padded) == 4 and sdnq_amd.merge_lora(b_model) == 4
    same_tensors(a_model, b_model)


@pytest.mark.parametrize("name", ("int8_rowwise", "uint4_g64"))
def test_a_zero_up_merges_to_the_requantization_of_the_weight(name, gpu_device):
    """up == 0: e is w32 itself, so the merged tensors are the quantizer's on the dequantized weight -- not necessarily the old codes (a
    lossless identity is not asserted)."""
    layer = CASES[name][0](gpu_device)
    dq, qw = layer.sdnq_dequantizer, LIN._state(layer).qw
    up, down = factors(qw.n, qw.k, 8, dq.result_dtype, gpu_device)
    want = ops.quantize_weight(ops.dequant(qw, torch.float32, 0, use_svd=False), dq.weights_dtype, qw.group_size)
    lora._merge_layer(layer, down, torch.zeros_like(up), 1.0, None)
    qw2 = LIN._state(layer).qw
    assert qw2 is not qw
    assert torch.equal(qw2.keep[0].contiguous().view(torch.uint8).reshape(-1), want[0].contiguous().view(torch.uint8).reshape(-1))
    assert torch.equal(layer.scale.float().reshape(-1), want[1].reshape(-1))
    if want[2] is not None:
        assert torch.equal(layer.zero_point.float().reshape(-1), want[2].reshape(-1))


@pytest.mark.parametrize("name", ("int8_rowwise", "uint4_g64"))
def test_the_composition_route_returns_the_fused_bits_on_exact_operands(name, gpu_device, monkeypatch):
    """The layer's tensors are overwritten with the planted codes and power-of-two scales of tests/dora_util.py, for which e is exact in
    float32 in any order: dequant + addmm + quantize_weight must then give what the fused kernel gives, bit for bit."""
    layer = CASES[name][0](gpu_device)
    dq = layer.sdnq_dequantizer
    n, k = dq.out_features, dq.in_features
    fmt = D.Fmt(dq.weights_dtype, dq.group_size if dq.group_size > 0 else 0)
    wt = D.plant_weight(fmt, n, k, seed=40)
    t32 = lambda a, like: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(like.shape).to(like.dtype).to(gpu_device)  # noqa: E731
    with torch.no_grad():
        codes = torch.from_numpy(wt.stored).to(gpu_device)
        if dq.weight_is_transposed:
            layer.weight.copy_(codes.view(torch.int8).reshape(n, k).t())
        else:
            layer.weight.copy_(codes.view(layer.weight.dtype).reshape(layer.weight.shape))
        layer.scale.copy_(t32(wt.scale, layer.scale))
        if wt.zp is not None:
            layer.zero_point.copy_(t32(wt.zp, layer.zero_point))
    w, _, _ = stored(layer)
    assert np.array_equal(w, wt.w), "the planted weight as the layer decodes it"
    up, down = D.plant_factors(n, k, 16, wt.er, seed=41)
    D.normsq_expected(wt.w, up, down, D.SCALE, wt.er)  # asserts the exactness of e
    dt = dq.result_dtype
    up, down = (torch.from_numpy(a.astype(np.float32)).to(dt).to(gpu_device) for a in (up, down))
    other = copy.deepcopy(layer)
    assert lora._merge_layer(layer, down, up, D.SCALE, None) == "fused"
    monkeypatch.setattr(lora, "_MERGE_FORCE_COMPOSITION", True)
    assert lora._merge_layer(other, down, up, D.SCALE, None) == "composed"
    for f in FIELDS:
        ta, tb = getattr(layer, f), getattr(other, f)
        if ta is not None:
            assert ta.stride() == tb.stride() and torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8)), f
