"""DoRA on the Linear adapters, host side: the five new exports and their argument checks, and add_lora(use_dora=True) / remove_lora /
lora_state_dict / load_lora_state_dict on a model built on the CPU (the initial norm comes from a stand-in for the norm kernel)."""
import ctypes
import importlib
import warnings

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, lora
from tests import dora_util as D
from tests.test_lora_host import toy_model

NEW = {"sdnq_hip_dora_normsq": 8, "sdnq_hip_dora_normsq_dense": 11, "sdnq_hip_lowrank_add_dora": 12, "sdnq_hip_dora_bwd_workspace_bytes": 2,
       "sdnq_hip_dora_bwd": 14}


def test_the_five_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    for name, arity in NEW.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(raw, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name
    assert raw.sdnq_hip_dora_bwd_workspace_bytes.restype is ctypes.c_int64
    assert "dora" in {u[0] for u in importlib.import_module("sdnq_amd._build").UNITS}
    assert issubclass(lora.QuantizedLinearDoRA, torch.autograd.Function)


def test_the_slab_and_the_chunk_are_constants_of_the_source():
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    ws = raw.sdnq_hip_dora_bwd_workspace_bytes
    assert D.constants_in_source() == {"DB_SLAB": D.DB_SLAB, "DN_KC": D.DN_KC}
    assert ws(D.DB_SLAB, 16) == 0 and ws(1, 16) == 0
    assert ws(D.DB_SLAB + 1, 16) == 2 * 16 * 4 and ws(675, 72) == 3 * 72 * 4
    assert ws(0, 16) == -3 and ws(5, 12) == -3


def test_argument_validation_without_gpu():
    """Validation runs before any launch, so the status codes are observable without a device."""
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    dense = raw.sdnq_hip_dora_normsq_dense
    ok = dict(wd=p, dt=_lib.BF16, n=8, k=16, ldw=16, up=p, down=p, rank=8, scale=0.5, out=p, stream=None)

    def rc(**broken):
        return dense(*{**ok, **broken}.values())
    assert rc(wd=None) == -1 and rc(out=None) == -1 and rc(up=None) == -1 and rc(down=None) == -1
    assert rc(dt=_lib.F32) == -2
    assert rc(k=24, ldw=24) == -3 and rc(n=12) == -3 and rc(rank=12) == -3 and rc(rank=264) == -3 and rc(ldw=8) == -3 and rc(n=0) == -3
    assert rc(wd=p + 8) == -4 and rc(up=p + 8) == -4 and rc(down=p + 2) == -4 and rc(ldw=20) == -4 and rc(out=p + 2) == -4
    w = _lib.SdnqWeight(weight=p, scale=p, n=8, k=16, group_size=16, storage=_lib.ST_RAW8, kind=_lib.KIND_INT, bits=8)
    codes = raw.sdnq_hip_dora_normsq
    assert codes(None, None, None, _lib.BF16, 0, 1.0, p, None) == -1
    assert codes(ctypes.byref(w), p, None, _lib.BF16, 8, 1.0, p, None) == -1                       # one factor without the other
    assert codes(ctypes.byref(w), p, p, _lib.F32, 8, 1.0, p, None) == -2
    assert codes(ctypes.byref(w), p, p, _lib.BF16, 12, 1.0, p, None) == -3
    w.svd_up, w.svd_down, w.svd_rank = p, p, 8
    assert codes(ctypes.byref(w), p, p, _lib.BF16, 8, 1.0, p, None) == _lib.ERR_UNSUPPORTED        # SVD factors: the dense form
    add = raw.sdnq_hip_lowrank_add_dora
    oka = dict(t=p, up=p, dt=_lib.BF16, rank=16, scale=1.0, y=p, m=5, n=16, ldy=16, c=p, bias=None, stream=None)

    def ra(**broken):
        return add(*{**oka, **broken}.values())
    assert ra(c=None) == -1 and ra(t=None) == -1 and ra(dt=_lib.F32) == -2 and ra(rank=12) == -3 and ra(n=12, ldy=12) == -3
    assert ra(c=p + 4) == -4 and ra(bias=p + 2) == -4
    bwd = raw.sdnq_hip_dora_bwd
    okb = dict(dy=p, lddy=16, y=p, ldy=16, bias=None, c=p, dt=_lib.F16, m=5, n=16, g=p, q=p, ws=None, wsb=0, stream=None)

    def rb(**broken):
        return bwd(*{**okb, **broken}.values())
    assert rb(dy=None) == -1 and rb(c=None) == -1 and rb(g=None) == -1 and rb(y=None) == -1
    assert rb(dt=_lib.F32) == -2 and rb(n=12, lddy=12, ldy=12) == -3 and rb(lddy=8) == -3 and rb(m=0) == -3
    assert rb(dy=p + 8) == -4 and rb(lddy=20) == -4 and rb(g=p + 2) == -4 and rb(c=p + 4) == -4
    many = D.DB_SLAB + 1                                                             # two slabs: the workspace is needed ...
    assert rb(m=many) == -1 and rb(m=many, ws=p, wsb=2 * 16 * 4 - 1) == -3 and rb(m=many, ws=p + 4, wsb=1 << 12) == -4


@pytest.fixture
def norm_stand_in(monkeypatch):
    """The norm kernel needs a device: on the CPU the row norms come from the layer's own stored int8 codes and scales."""
    def normsq(layer, down, up):
        w = layer.weight.detach().float().reshape(layer.sdnq_dequantizer.out_features, -1) * layer.scale.detach().float().reshape(-1, 1)
        if up is not None:
            w = w + layer.lora_scale * up.float() @ down.float()
        return (w * w).sum(1)
    monkeypatch.setattr(lora, "_layer_normsq", normsq)


def test_add_lora_use_dora_registers_the_magnitude(norm_stand_in):
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = sdnq_amd.add_lora(m, rank=16, alpha=32, seed=7, dtype=torch.bfloat16, use_dora=True)
    assert res == 2
    for name, n_out in (("q", 48), ("k", 72)):
        mod = getattr(m, name)
        assert isinstance(mod.lora_magnitude, torch.nn.Parameter) and mod.lora_magnitude.shape == (n_out,)
        assert mod.lora_magnitude.dtype == torch.float32 and mod.lora_magnitude.requires_grad and mod.lora_dora is True   # float32 whatever dtype= says
        assert bool((mod.lora_magnitude > 0).all()) and mod.forward_func.__module__ == "sdnq_amd.lora"
        assert torch.equal(mod.lora_magnitude.detach(), torch.sqrt(lora._layer_normsq(mod, None, None)))
    assert [id(p) for p in res.parameters] == [id(m.q.lora_down), id(m.q.lora_up), id(m.q.lora_magnitude),
                                               id(m.k.lora_down), id(m.k.lora_up), id(m.k.lora_magnitude)]
    assert sdnq_amd.remove_lora(m) == 2
    for name in ("q", "k"):
        mod = getattr(m, name)
        assert not any(hasattr(mod, a) for a in ("lora_down", "lora_up", "lora_scale", "lora_dropout", "lora_magnitude", "lora_dora"))
        assert not any("lora" in k for k, _ in mod.named_parameters())


def test_a_zero_weight_row_is_skipped_with_its_sentence(norm_stand_in):
    m = toy_model()
    with torch.no_grad():
        m.k.weight.reshape(72, -1)[5].zero_()
    before = m.k.forward_func
    with pytest.warns(UserWarning, match="got no adapter"):
        res = sdnq_amd.add_lora(m, rank=8, use_dora=True)
    why = dict(res.skipped)
    assert res == 1 and "k" in why and "all-zero" in why["k"] and "DoRA" in why["k"]
    assert m.k.forward_func is before and not hasattr(m.k, "lora_down") and not hasattr(m.k, "lora_magnitude")
    assert hasattr(m.q, "lora_magnitude")


def test_convs_with_dora_raise_before_any_module_is_touched(norm_stand_in):
    m = toy_model()
    before = {n: mod.forward_func for n, mod in m.named_modules() if hasattr(mod, "forward_func")}
    with pytest.raises(NotImplementedError, match="DoRA on conv"):
        sdnq_amd.add_lora(m, rank=8, convs=True, use_dora=True)
    assert all(mod.forward_func is before[n] for n, mod in m.named_modules() if hasattr(mod, "forward_func"))
    assert not any("lora" in k for k, _ in m.named_parameters())


def test_state_dict_round_trip_and_the_three_key_forms(norm_stand_in):
    m, other = toy_model(), toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, seed=1, use_dora=True)
        sdnq_amd.add_lora(other, rank=8, seed=2, use_dora=True)
    with torch.no_grad():
        m.q.lora_up.copy_(torch.randn(48, 8))
        m.q.lora_magnitude.mul_(1.5)
    sd = sdnq_amd.lora_state_dict(m)
    assert set(sd) == {f"{n}.{k}" for n in ("q", "k") for k in ("lora_A.weight", "lora_B.weight", "lora_magnitude_vector.weight")}
    assert sd["q.lora_magnitude_vector.weight"].dtype == torch.float32 and not any(v.requires_grad for v in sd.values())
    assert sdnq_amd.load_lora_state_dict(other, {k: v.clone() for k, v in sd.items()}) == 2
    assert torch.equal(other.q.lora_magnitude, m.q.lora_magnitude) and torch.equal(other.k.lora_magnitude, m.k.lora_magnitude)
    assert torch.equal(other.q.lora_up, m.q.lora_up)
    for form in (".lora_magnitude_vector.default.weight", ".lora_magnitude_vector.default"):       # PEFT's two spellings
        peft = {}
        for k, v in sd.items():
            if "magnitude" in k:
                peft["base_model.model." + k.replace(".lora_magnitude_vector.weight", form)] = v * 2
            else:
                peft["base_model.model." + k.replace(".weight", ".default.weight")] = v
        assert sdnq_amd.load_lora_state_dict(other, peft) == 2 and torch.equal(other.q.lora_magnitude, m.q.lora_magnitude * 2)
    with pytest.raises(KeyError, match="lora_magnitude_vector"):                                    # a DoRA layer needs its magnitude
        sdnq_amd.load_lora_state_dict(other, {k: v for k, v in sd.items() if k != "k.lora_magnitude_vector.weight"})
    with pytest.raises(ValueError, match="shape"):
        sdnq_amd.load_lora_state_dict(other, {**sd, "q.lora_magnitude_vector.weight": torch.zeros(40)})
    plain = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(plain, rank=8, seed=3)
    with pytest.raises(KeyError, match="magnitude"):                                                # a magnitude key on a model without DoRA
        sdnq_amd.load_lora_state_dict(plain, sd)


def test_the_default_leaves_keys_and_parameters_as_they_are():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = sdnq_amd.add_lora(m, rank=8, seed=1)
    assert set(sdnq_amd.lora_state_dict(m)) == {"q.lora_A.weight", "q.lora_B.weight", "k.lora_A.weight", "k.lora_B.weight"}
    assert [id(p) for p in res.parameters] == [id(m.q.lora_down), id(m.q.lora_up), id(m.k.lora_down), id(m.k.lora_up)]
    assert not hasattr(m.q, "lora_magnitude") and not hasattr(m.q, "lora_dora")
    assert m.q.forward_func.__name__.endswith("_with_lora")
