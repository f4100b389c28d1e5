"""Trainable low-rank adapters, host side: the three new exports and their argument checks, the checks of the ops wrappers, and
sdnq_amd.add_lora / remove_lora / lora_state_dict / load_lora_state_dict on a model built on the CPU."""
import copy
import ctypes
import importlib
import math
import warnings

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, lora, ops, training as T
from tests import lora_util as L

NEW = {"sdnq_hip_lowrank_add": 10, "sdnq_hip_lowrank_grad_workspace_bytes": 3, "sdnq_hip_lowrank_grad": 14}


def test_the_three_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    for name, arity in NEW.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(raw, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name
    assert raw.sdnq_hip_lowrank_grad_workspace_bytes.restype is ctypes.c_int64
    units = {u[0]: u[1] for u in importlib.import_module("sdnq_amd._build").UNITS}
    assert "kernarg-preload" in units["lowrank_train"]
    assert sdnq_amd.add_lora is lora.add_lora and sdnq_amd.remove_lora is lora.remove_lora
    assert sdnq_amd.lora_state_dict is lora.lora_state_dict and sdnq_amd.load_lora_state_dict is lora.load_lora_state_dict


def test_the_slab_is_a_constant_of_the_source():
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    ws = raw.sdnq_hip_lowrank_grad_workspace_bytes
    assert L.slab_constant_in_source() == L.LRG_SLAB
    assert ws(L.LRG_SLAB, 16, 8) == 0 and ws(1, 16, 8) == 0                      # one slab: no workspace
    assert ws(L.LRG_SLAB + 1, 16, 8) == 2 * 16 * 8 * 4                           # float32 [slab][P][rank]
    assert ws(4100, 1288, 64) == -(-4100 // L.LRG_SLAB) * 1288 * 64 * 4
    assert ws(0, 16, 8) == -3 and ws(5, 12, 8) == -3 and ws(5, 16, 12) == -3 and ws(5, 16, 264) == -3 and ws(5, 16, 0) == -3


def test_argument_validation_without_gpu():
    """Validation runs before any launch, so the status codes are observable without a device."""
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    add = raw.sdnq_hip_lowrank_add
    ok = dict(t=p, up=p, dt=_lib.BF16, rank=16, scale=1.0, y=p, m=5, n=16, ldy=16, stream=None)

    def rc(**broken):
        return add(*{**ok, **broken}.values())
    assert rc(t=None) == -1 and rc(up=None) == -1 and rc(y=None) == -1
    assert rc(dt=_lib.F32) == -2 and rc(dt=7) == -2
    assert rc(rank=12) == -3 and rc(rank=0) == -3 and rc(rank=264) == -3           # rank % 8, 8 <= rank <= 256
    assert rc(n=12, ldy=12) == -3 and rc(ldy=8) == -3 and rc(m=0) == -3            # n % 8, ldy < n
    assert rc(t=p + 8) == -4 and rc(up=p + 2) == -4 and rc(y=p + 8) == -4          # misaligned pointers
    assert rc(ldy=20) == -4                                                        # rows of 40 bytes
    grad = raw.sdnq_hip_lowrank_grad
    okg = dict(a=p, lda=16, b=p, dt=_lib.F16, m=5, p=16, rank=8, scale=1.0, out_t=0, out=p, odt=_lib.F32, ws=None, wsb=0, stream=None)

    def rg(**broken):
        return grad(*{**okg, **broken}.values())
    assert rg(a=None) == -1 and rg(b=None) == -1 and rg(out=None) == -1
    assert rg(dt=_lib.F32) == -2 and rg(odt=3) == -2 and rg(odt=-1) == -2
    assert rg(p=12, lda=12) == -3 and rg(lda=8) == -3 and rg(rank=12) == -3 and rg(rank=512) == -3 and rg(m=0) == -3 and rg(out_t=2) == -3
    assert rg(a=p + 8) == -4 and rg(b=p + 4) == -4 and rg(lda=20) == -4 and rg(out=p + 2) == -4
    many = L.LRG_SLAB + 1                                                           # two slabs: the workspace is needed
    assert rg(m=many) == -1                                                         # ... NULL
    assert rg(m=many, ws=p, wsb=2 * 16 * 8 * 4 - 1) == -3                           # ... too small
    assert rg(m=many, ws=p + 4, wsb=1 << 12) == -4                                  # ... misaligned


def test_ops_checks_name_what_is_wrong():
    bf = torch.bfloat16
    t, up, y = torch.zeros(5, 16, dtype=bf), torch.zeros(24, 16, dtype=bf), torch.zeros(5, 24, dtype=bf)
    err = _lib.SdnqHipError
    with pytest.raises(err, match="CPU"):
        ops.lowrank_add(t, up, y, 1.0)
    with pytest.raises(err, match="CPU"):
        ops.lowrank_grad(y, t, 1.0)
    with pytest.raises(err, match="float32"):
        ops.lowrank_add(t.float(), up.float(), y.float(), 1.0)
    with pytest.raises(err, match="float32"):
        ops.lowrank_grad(y.float(), t.float())
    with pytest.raises(err, match=r"up must have the dtype"):
        ops.lowrank_add(t, up.half(), y, 1.0)
    with pytest.raises(err, match=r"rank = 12"):
        ops.lowrank_add(t[:, :12].contiguous(), up[:, :12].contiguous(), y, 1.0)
    with pytest.raises(err, match=r"rank = 12"):
        ops.lowrank_grad(y, t[:, :12].contiguous())
    with pytest.raises(err, match=r"n = 20"):
        ops.lowrank_add(t, up[:20], y[:, :20], 1.0)
    with pytest.raises(err, match=r"p = 20"):
        ops.lowrank_grad(y[:, :20], t)
    with pytest.raises(err, match="y is misaligned"):
        ops.lowrank_add(t, up[:16], torch.zeros(5, 32, dtype=bf)[:, 4:20], 1.0)     # a column view that starts 8 bytes in
    with pytest.raises(err, match="a is misaligned"):
        ops.lowrank_grad(torch.zeros(5, 28, dtype=bf)[:, :24], t)                   # rows of 56 bytes
    with pytest.raises(err, match="t and up must be contiguous"):
        ops.lowrank_add(torch.zeros(5, 32, dtype=bf)[:, :16], up, y, 1.0)
    with pytest.raises(err, match=r"y \[M, N\]"):
        ops.lowrank_add(t, up, y[:4], 1.0)
    with pytest.raises(err, match="same rows"):
        ops.lowrank_grad(y, t[:4])
    # a single row: torch leaves the stride of the size-1 axis arbitrary, the library is given the row length -- the checks pass
    one = torch.zeros(24, dtype=bf).as_strided((1, 24), (3, 1))
    with pytest.raises(err, match="CPU"):
        ops.lowrank_add(t[:1], up, one, 1.0)
    with pytest.raises(err, match="CPU"):
        ops.lowrank_grad(one, t[:1])
    assert ops._ld(one) == 24 and ops._ld(y[:, :16]) == 24


def test_the_dropout_triple_has_the_order_of_the_entry_points_and_is_never_indexed():
    """One order for (threshold, seed, offset) from the draw to the library: the fields of ops._Dropout are the trailing dropout parameters
    of the three wrappers, in their order, and sdnq_amd/lora.py passes the triple on whole or splats it -- no subscript of a name `drop`."""
    import ast
    import inspect
    fields = ops._Dropout._fields
    assert fields == ("threshold", "seed", "offset")
    for fn in (ops.lowrank_add_dropout, ops.lowrank_grad_dropout, ops.lowrank_down_dropout):
        assert tuple(p for p in inspect.signature(fn).parameters if p in fields) == fields, fn.__name__
    with open(lora.__file__) as f:
        tree = ast.parse(f.read())
    indexed = [node.lineno for node in ast.walk(tree)
               if isinstance(node, ast.Subscript) and isinstance(node.value, ast.Name) and node.value.id == "drop"]
    assert indexed == [], indexed
    assert lora._scale(type("Layer", (), {"lora_scale": 2.0})(), ops._Dropout(16384, 7, 4)) == lora.dropout_scale(2.0, 16384)


class Toy(torch.nn.Module):
    def __init__(self, dtype=torch.bfloat16):
        super().__init__()
        self.emb = torch.nn.Embedding(64, 64)
        self.a = torch.nn.Linear(64, 64)          # stays float: not an SDNQ layer, not looked at
        self.q = torch.nn.Linear(64, 48)
        self.k = torch.nn.Linear(64, 72)
        self.odd = torch.nn.Linear(64, 44)        # N % 8 != 0
        self.f32 = torch.nn.Linear(64, 48)
        self.conv = torch.nn.Conv2d(16, 32, 3, padding=1)

    def forward(self, x):
        return self.q(self.a(x))


QUANTIZED = ("q", "k", "odd", "f32", "conv", "emb")


def toy_model():
    torch.manual_seed(0)
    m = Toy().to(torch.bfloat16)
    m.f32 = m.f32.float()
    cfg = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    for name in QUANTIZED:
        extra = {"conv": {"quant_conv": True}, "emb": {"quant_embedding": True}}.get(name, {})
        layer, _ = sdnq_amd.sdnq_quantize_layer(getattr(m, name), sdnq_amd.SDNQConfig(**cfg, **extra))
        setattr(m, name, layer)
    assert all(getattr(getattr(m, n), "sdnq_dequantizer", None) is not None for n in QUANTIZED)
    assert m.f32.sdnq_dequantizer.result_dtype == torch.float32
    return m


def test_add_lora_registers_skips_and_warns_once():
    m = toy_model()
    before = {n: getattr(m, n).forward_func for n in QUANTIZED}
    with pytest.warns(UserWarning, match="got no adapter") as rec:
        res = sdnq_amd.add_lora(m, rank=16, alpha=32, seed=7)
    assert len(rec) == 1
    assert isinstance(res, int) and res == 2 and res.added == 2
    why = dict(res.skipped)
    assert set(why) == {"odd", "f32", "conv", "emb"}
    assert "Conv2d" in why["conv"] and "Linear layers" in why["conv"]
    assert "Embedding" in why["emb"] and "Linear layers" in why["emb"]
    assert "float32" in why["f32"] and "bfloat16" in why["f32"]
    assert "8 | N" in why["odd"] and "N = 44" in why["odd"]
    assert all(n in str(rec[0].message) for n in why)
    assert all(getattr(m, n).forward_func is before[n] for n in why)
    for name, n_out in (("q", 48), ("k", 72)):
        mod = getattr(m, name)
        assert isinstance(mod.lora_down, torch.nn.Parameter) and isinstance(mod.lora_up, torch.nn.Parameter)
        assert mod.lora_down.shape == (16, 64) and mod.lora_up.shape == (n_out, 16)
        assert mod.lora_down.dtype == mod.lora_up.dtype == torch.bfloat16
        assert mod.lora_down.requires_grad and mod.lora_up.requires_grad
        assert not mod.lora_up.any() and mod.lora_scale == 2.0
        bound = 1 / math.sqrt(64)                  # nn.Linear's kaiming_uniform_(a = sqrt(5)) on fan_in = 64
        d = mod.lora_down.detach().float()
        assert float(d.abs().max()) <= bound * 1.01 and float(d.abs().max()) > 0.8 * bound and abs(float(d.mean())) < 0.02
        assert 0.8 * bound / math.sqrt(3) < float(d.std()) < 1.2 * bound / math.sqrt(3)
        assert mod.forward_func is not before[name] and mod.forward_func.__module__ == "sdnq_amd.lora"
        assert mod.forward_func._sdnq_lora_base is before[name]
        assert {"lora_down", "lora_up"} <= {k for k, _ in mod.named_parameters()}
    assert not torch.equal(m.q.lora_down, m.k.lora_down)
    assert [id(p) for p in res.parameters] == [id(m.q.lora_down), id(m.q.lora_up), id(m.k.lora_down), id(m.k.lora_up)]
    # the same seed draws the same factors, another one does not; float32 master weights; the default scale is 1
    m2, m3 = toy_model(), toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r2 = sdnq_amd.add_lora(m2, rank=16, dtype=torch.float32, seed=7)
        sdnq_amd.add_lora(m3, rank=16, seed=8)
        again = sdnq_amd.add_lora(m2, rank=16)
    assert m2.q.lora_down.dtype == torch.float32 and m2.q.lora_scale == 1.0 and r2.added == 2
    assert torch.equal(m2.q.lora_down.to(torch.bfloat16), m.q.lora_down) and torch.equal(m2.k.lora_down.to(torch.bfloat16), m.k.lora_down)
    assert not torch.equal(m3.q.lora_down, m.q.lora_down)
    assert again.added == 0 and "already" in dict(again.skipped)["q"]              # not wrapped twice
    with pytest.raises(ValueError, match="rank = 12"):
        sdnq_amd.add_lora(toy_model(), rank=12)
    with pytest.raises(ValueError, match="float64"):
        sdnq_amd.add_lora(toy_model(), dtype=torch.float64)


def test_targets_select_by_substring_or_predicate():
    m = toy_model()
    res = sdnq_amd.add_lora(m, rank=8, targets=["q"])                              # nothing skipped: no warning
    assert res.added == 1 and res.skipped == [] and hasattr(m.q, "lora_down") and not hasattr(m.k, "lora_down")
    m = toy_model()
    with pytest.warns(UserWarning, match="emb"):
        res = sdnq_amd.add_lora(m, rank=8, targets=lambda name: name in ("k", "emb"))
    assert res.added == 1 and [n for n, _ in res.skipped] == ["emb"] and hasattr(m.k, "lora_down") and not hasattr(m.q, "lora_down")


def test_enable_input_grad_afterwards_leaves_the_adapter_layers_alone():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, targets=["q"])
        wrapped = m.q.forward_func
        res = sdnq_amd.enable_input_grad(m)
    why = dict(res.skipped)
    assert "q" in why and "does not run on the MI355X forwards" in why["q"]
    assert m.q.forward_func is wrapped and res.enabled == 2                        # k and f32 are switched, q keeps its adapter forward
    assert sdnq_amd.enable_input_grad(m, enabled=False) == 2 and m.q.forward_func is wrapped


def test_add_lora_unwraps_enable_input_grad_and_remove_lora_restores():
    m = toy_model()
    inference = {n: getattr(m, n).forward_func for n in QUANTIZED}
    compile_plans = {n: getattr(m, n).__dict__.get("_sdnq_hip_plan") for n in ("q", "k")}
    assert compile_plans["q"] is not None                                          # q traces as rowquant + matmul operators under torch.compile
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert sdnq_amd.enable_input_grad(m) == 3
        switched = {n: getattr(m, n).forward_func for n in QUANTIZED}
        assert sdnq_amd.add_lora(m, rank=8) == 2
    assert m.q.forward_func._sdnq_lora_base is inference["q"] and m.k.forward_func._sdnq_lora_base is inference["k"]
    assert m.q.__dict__["_sdnq_hip_plan"] is None and m.k.__dict__["_sdnq_hip_plan"] is None   # ... with an adapter as the whole-layer operator
    # whoever derives the plan again finds none while the adapter is on: the handle (accelerate, apply_sdnq_options_to_model), a deepcopy
    from sdnq_amd import torch_ops
    assert torch_ops.layer_plan(m.q) is None
    torch_ops.layer_handle(m.q)
    assert m.q.__dict__["_sdnq_hip_plan"] is None
    twin = copy.deepcopy(m)
    assert twin.q.__dict__["_sdnq_hip_plan"] is None and twin.q.forward_func._sdnq_lora_base is inference["q"]
    assert twin.q.lora_down is not m.q.lora_down and torch.equal(twin.q.lora_down, m.q.lora_down)
    assert sdnq_amd.remove_lora(m) == 2
    assert all(getattr(m, n).forward_func is switched[n] for n in QUANTIZED)       # the very objects they had before
    assert all(getattr(m, n).__dict__["_sdnq_hip_plan"] == compile_plans[n] for n in compile_plans)
    for name in ("q", "k"):
        mod = getattr(m, name)
        assert not any(hasattr(mod, a) for a in ("lora_down", "lora_up", "lora_scale"))
        assert not any("lora" in k for k, _ in mod.named_parameters())
    assert sdnq_amd.remove_lora(m) == 0 and sdnq_amd.lora_state_dict(m) == {}


def test_a_forward_re_pointed_afterwards_drops_the_adapter_and_remove_lora_tidies_up():
    m = toy_model()
    plan = m.q.__dict__["_sdnq_hip_plan"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, targets=["q"])
        sdnq_amd.accelerate(m)
    # eager and compiled agree: no adapter forward, the layer's own compile plan
    assert m.q.forward_func.__module__ == "sdnq_amd.linear" and m.q.__dict__["_sdnq_hip_plan"] == plan
    assert hasattr(m.q, "lora_down") and sdnq_amd.lora_state_dict(m) == {}
    assert sdnq_amd.remove_lora(m) == 1 and not hasattr(m.q, "lora_down") and m.q.forward_func.__module__ == "sdnq_amd.linear"


def test_state_dict_round_trips_under_the_peft_names():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, seed=1)
    with torch.no_grad():
        m.q.lora_up.copy_(torch.randn(48, 8))
        m.k.lora_up.copy_(torch.randn(72, 8))
    sd = sdnq_amd.lora_state_dict(m)
    assert set(sd) == {"q.lora_A.weight", "q.lora_B.weight", "k.lora_A.weight", "k.lora_B.weight"}
    assert sd["q.lora_A.weight"].shape == (8, 64) and sd["k.lora_B.weight"].shape == (72, 8)
    assert not any(v.requires_grad for v in sd.values())
    other = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(other, rank=8, seed=2)
    assert sdnq_amd.load_lora_state_dict(other, {k: v.clone() for k, v in sd.items()}) == 2
    for name in ("q", "k"):
        assert torch.equal(getattr(other, name).lora_down, getattr(m, name).lora_down)
        assert torch.equal(getattr(other, name).lora_up, getattr(m, name).lora_up)
    # PEFT's own spelling: a base_model.model. prefix and the adapter name
    peft = {"base_model.model." + k.replace(".weight", ".default.weight"): v * 2 for k, v in sd.items()}
    assert sdnq_amd.load_lora_state_dict(other, peft) == 2 and torch.equal(other.q.lora_up, m.q.lora_up * 2)
    with pytest.raises(KeyError, match="odd"):
        sdnq_amd.load_lora_state_dict(other, {**sd, "odd.lora_A.weight": sd["q.lora_A.weight"]})
    with pytest.raises(KeyError, match="both"):
        sdnq_amd.load_lora_state_dict(other, {k: v for k, v in sd.items() if k != "k.lora_B.weight"})
    with pytest.raises(ValueError, match="shape"):
        sdnq_amd.load_lora_state_dict(other, {**sd, "q.lora_A.weight": torch.zeros(16, 64)})
    with pytest.raises(KeyError, match="not a"):
        sdnq_amd.load_lora_state_dict(other, {"q.weight": torch.zeros(1)})


def test_cpu_forward_raises_with_and_without_a_graph():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8)
    x = torch.randn(40, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        m.q(x)                                     # the factors require grad: QuantizedLinearLoRA
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        with torch.no_grad():
            m.q(x)                                 # LoRA inference
    assert issubclass(lora.QuantizedLinearLoRA, torch.autograd.Function)
    assert T.scratch_bytes.__module__ == "sdnq_amd.training"
