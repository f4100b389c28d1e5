"""Low-rank adapters on frozen quantized conv layers, host side: the three new exports and their argument checks, the checks of the ops
wrappers, and sdnq_amd.add_lora(..., convs=True) / remove_lora / lora_state_dict / load_lora_state_dict on a model built on the CPU."""
import ctypes
import importlib
import math
import warnings

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, lora, ops, training as T
from tests import conv_lora_util as C
from tests import test_lora_host as H

NEW = {"sdnq_hip_conv_lowrank_down": 18, "sdnq_hip_conv_lowrank_grad_workspace_bytes": 13, "sdnq_hip_conv_lowrank_grad": 22}


def test_the_three_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    for name, arity in NEW.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(raw, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name
    assert raw.sdnq_hip_conv_lowrank_grad_workspace_bytes.restype is ctypes.c_int64
    assert "conv_lowrank" in {u[0] for u in importlib.import_module("sdnq_amd._build").UNITS}
    assert issubclass(lora.QuantizedConvLoRA, torch.autograd.Function)


def test_the_slab_is_a_constant_of_the_source():
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    ws = raw.sdnq_hip_conv_lowrank_grad_workspace_bytes
    assert C.slab_constant_in_source() == C.CLG_SLAB
    geo = dict(b=1, c=16, h=16, w=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, rank=8)

    def nbytes(**other):
        return ws(*{**geo, **other}.values())
    assert nbytes() == 0 and nbytes(h=1, kh=1, ph=0, w=5) == 0                     # M = 256 = one slab: no workspace
    assert nbytes(b=3, h=15, w=15) == 3 * 144 * 8 * 4                              # M = 675: float32 [slab][K][rank]
    assert nbytes(h=17) == 2 * 144 * 8 * 4 and nbytes(b=2, sh=2, sw=2) == 0       # M = 272; 2 x 8 x 8 = 128
    assert nbytes(b=0) == -3 and nbytes(rank=12) == -3 and nbytes(rank=264) == -3 and nbytes(c=3) == -3    # K = 27
    assert nbytes(h=1, ph=0) == -3 and nbytes(sh=0) == -3 and nbytes(dw=0) == -3 and nbytes(pw=-1) == -3   # an empty output; bad steps


def test_argument_validation_without_gpu():
    """Validation runs before any launch, so the status codes are observable without a device."""
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    down = raw.sdnq_hip_conv_lowrank_down
    ok = dict(x=p, dt=_lib.BF16, b=2, c=16, h=7, w=9, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, down=p, rank=16, t=p, stream=None)

    def rc(**broken):
        return down(*{**ok, **broken}.values())
    assert rc(x=None) == -1 and rc(down=None) == -1 and rc(t=None) == -1
    assert rc(dt=_lib.F32) == -2 and rc(dt=7) == -2
    assert rc(rank=12) == -3 and rc(rank=0) == -3 and rc(rank=264) == -3           # rank % 8, 8 <= rank <= 256
    assert rc(c=3) == -3 and rc(c=4, kh=1, kw=1, ph=0, pw=0) == -3                 # C kh kw % 8
    assert rc(b=0) == -3 and rc(c=0) == -3 and rc(h=0) == -3 and rc(w=-1) == -3 and rc(kh=0) == -3 and rc(kw=0) == -3
    assert rc(sh=0) == -3 and rc(sw=-1) == -3 and rc(ph=-1) == -3 and rc(dh=0) == -3 and rc(dw=0) == -3
    assert rc(h=1, ph=0) == -3 and rc(w=4, pw=0, dw=3) == -3                       # no output position
    assert rc(x=p + 8) == -4 and rc(down=p + 2) == -4 and rc(t=p + 8) == -4        # misaligned pointers
    grad = raw.sdnq_hip_conv_lowrank_grad
    okg = dict(x=p, dt=_lib.F16, b=2, c=16, h=7, w=9, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, g=p, rank=8, scale=1.0, out=p,
               odt=_lib.F32, ws=None, wsb=0, stream=None)

    def rg(**broken):
        return grad(*{**okg, **broken}.values())
    assert rg(x=None) == -1 and rg(g=None) == -1 and rg(out=None) == -1
    assert rg(dt=_lib.F32) == -2 and rg(odt=3) == -2 and rg(odt=-1) == -2
    assert rg(rank=12) == -3 and rg(rank=512) == -3 and rg(c=3) == -3 and rg(b=0) == -3 and rg(sh=0) == -3 and rg(h=1, ph=0) == -3
    assert rg(x=p + 8) == -4 and rg(g=p + 4) == -4 and rg(out=p + 4) == -4
    many = dict(b=5)                                                                # M = 315: two slabs, the workspace is needed
    assert rg(**many) == -1                                                         # ... NULL
    assert rg(**many, ws=p, wsb=2 * 144 * 8 * 4 - 1) == -3                          # ... too small
    assert rg(**many, ws=p + 4, wsb=1 << 14) == -4                                  # ... misaligned


def test_ops_checks_name_what_is_wrong():
    bf = torch.bfloat16
    x, down, g = torch.zeros(2, 16, 7, 9, dtype=bf), torch.zeros(16, 144, dtype=bf), torch.zeros(126, 16, dtype=bf)
    geo = ((3, 3), (1, 1), (1, 1), (1, 1))
    err = _lib.SdnqHipError
    with pytest.raises(err, match="CPU"):
        ops.conv_lowrank_down(x, down, *geo)
    with pytest.raises(err, match="CPU"):
        ops.conv_lowrank_grad(x, g, *geo)
    with pytest.raises(err, match="float32"):
        ops.conv_lowrank_down(x.float(), down.float(), *geo)
    with pytest.raises(err, match="float32"):
        ops.conv_lowrank_grad(x.float(), g.float(), *geo)
    with pytest.raises(err, match="dtype of x"):
        ops.conv_lowrank_down(x, down.half(), *geo)
    with pytest.raises(err, match=r"rank = 12"):
        ops.conv_lowrank_down(x, down[:12], *geo)
    with pytest.raises(err, match=r"rank = 12"):
        ops.conv_lowrank_grad(x, g[:, :12].contiguous(), *geo)
    with pytest.raises(err, match=r"C \* kh \* kw = 144"):
        ops.conv_lowrank_down(x, torch.zeros(16, 136, dtype=bf), *geo)
    with pytest.raises(err, match=r"H_out \* W_out = 126"):
        ops.conv_lowrank_grad(x, g[:120], *geo)
    with pytest.raises(err, match=r"% 8 == 0 \(got 27\)"):
        ops.conv_lowrank_down(x[:, :3], torch.zeros(16, 27, dtype=bf), *geo)
    with pytest.raises(err, match="empty"):
        ops.conv_lowrank_down(x, down, (3, 3), (1, 1), (0, 0), (4, 1))
    with pytest.raises(err, match=r"\[B, C, H, W\]"):
        ops.conv_lowrank_down(x[0], down, *geo)


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q = torch.nn.Linear(64, 48)
        self.conv = torch.nn.Conv2d(16, 32, 3, padding=1)
        self.conv1d = torch.nn.Conv1d(16, 32, 5, stride=2, padding=2)
        self.grouped = torch.nn.Conv2d(32, 32, 3, padding=1, groups=2)
        self.conv3d = torch.nn.Conv3d(16, 16, 3, padding=1)
        self.f32 = torch.nn.Conv2d(16, 32, 3, padding=1)
        self.same = torch.nn.Conv2d(16, 32, 3, padding="same")
        self.reflect = torch.nn.Conv2d(16, 32, 3, padding=1, padding_mode="reflect")
        self.up = torch.nn.ConvTranspose2d(16, 16, 2, stride=2)
        self.emb = torch.nn.Embedding(64, 64)


QUANTIZED = ("q", "conv", "conv1d", "grouped", "conv3d", "f32", "same", "reflect", "up", "emb")


def toy_model():
    torch.manual_seed(0)
    m = Toy().to(torch.bfloat16)
    m.f32 = m.f32.float()
    cfg = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, quant_conv=True, quant_embedding=True)
    for name in QUANTIZED:
        layer, _ = sdnq_amd.sdnq_quantize_layer(getattr(m, name), sdnq_amd.SDNQConfig(**cfg))
        setattr(m, name, layer)
    assert all(getattr(getattr(m, n), "sdnq_dequantizer", None) is not None for n in QUANTIZED)
    return m


def _quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def test_add_lora_without_convs_is_todays_result():
    m = H.toy_model()
    before = {n: getattr(m, n).forward_func for n in H.QUANTIZED}
    res = _quiet(sdnq_amd.add_lora, m, rank=16, alpha=32, seed=7)
    again = H.toy_model()
    explicit = _quiet(sdnq_amd.add_lora, again, rank=16, alpha=32, seed=7, convs=False)
    assert res == explicit == 2 and res.skipped == explicit.skipped
    why = dict(res.skipped)
    assert set(why) == {"odd", "f32", "conv", "emb"}
    assert why["conv"] == "Conv2d: adapters are built for quantized Linear layers (conv, transposed-conv and embedding layers are not)"
    assert why["conv"] == lora.lora_unsupported_reason(m.conv) and m.conv.forward_func is before["conv"]
    assert not hasattr(m.conv, "lora_down") and torch.equal(m.q.lora_down, again.q.lora_down)
    # the same draws as before the conv layers existed: q and k in module order
    gen = torch.Generator().manual_seed(7)
    bound = 1 / math.sqrt(64)
    for mod in (m.q, m.k):
        want = torch.empty((16, 64), dtype=torch.float32).uniform_(-bound, bound, generator=gen).to(torch.bfloat16)
        assert torch.equal(mod.lora_down, want)


def test_add_lora_convs_registers_the_peft_shapes_and_skips_with_sentences():
    m = toy_model()
    before = {n: getattr(m, n).forward_func for n in QUANTIZED}
    with pytest.warns(UserWarning, match="got no adapter") as rec:
        res = sdnq_amd.add_lora(m, rank=16, alpha=32, seed=7, convs=True)
    assert len(rec) == 1
    why = dict(res.skipped)
    assert res == 3 and set(why) == {"grouped", "conv3d", "f32", "same", "reflect", "up", "emb"}, why
    assert "groups = 2" in why["grouped"] and "groups == 1" in why["grouped"]
    assert "Conv3d" in why["conv3d"] and "Conv1d and Conv2d" in why["conv3d"]
    assert "float32" in why["f32"] and "bfloat16" in why["f32"]
    assert "padding='same'" in why["same"] and "padding_mode='reflect'" in why["reflect"]
    assert "ConvTranspose2d" in why["up"] and "transposed-conv" in why["up"]
    assert "Embedding" in why["emb"] and "embedding" in why["emb"]
    assert all(getattr(m, n).forward_func is before[n] for n in why)
    assert all(lora.lora_unsupported_reason(getattr(m, n), convs=True) == why[n] for n in why)
    for name, down_shape, up_shape, fan_in in (("conv", (16, 16, 3, 3), (32, 16, 1, 1), 144), ("conv1d", (16, 16, 5), (32, 16, 1), 80)):
        mod = getattr(m, name)
        assert isinstance(mod.lora_down, torch.nn.Parameter) and isinstance(mod.lora_up, torch.nn.Parameter)
        assert mod.lora_down.shape == down_shape and mod.lora_up.shape == up_shape
        assert mod.lora_down.dtype == mod.lora_up.dtype == torch.bfloat16 and mod.lora_down.requires_grad and mod.lora_up.requires_grad
        assert not mod.lora_up.any() and mod.lora_scale == 2.0
        bound = 1 / math.sqrt(fan_in)              # kaiming_uniform_(a = sqrt(5)) on fan_in = C_in * prod(kernel)
        d = mod.lora_down.detach().float()
        assert 0.8 * bound < float(d.abs().max()) <= bound * 1.01 and abs(float(d.mean())) < 0.02
        assert 0.8 * bound / math.sqrt(3) < float(d.std()) < 1.2 * bound / math.sqrt(3)
        assert mod.forward_func is not before[name] and mod.forward_func.__module__ == "sdnq_amd.lora"
        assert mod.forward_func._sdnq_lora_base is before[name]
    assert [id(p) for p in res.parameters] == [id(p) for mod in (m.q, m.conv, m.conv1d) for p in (mod.lora_down, mod.lora_up)]
    # drawn from the seed in module order, Linear and conv layers alike
    gen = torch.Generator().manual_seed(7)
    for mod, shape, fan_in in ((m.q, (16, 64), 64), (m.conv, (16, 16, 3, 3), 144), (m.conv1d, (16, 16, 5), 80)):
        b = 1 / math.sqrt(fan_in)
        assert torch.equal(mod.lora_down, torch.empty(shape, dtype=torch.float32).uniform_(-b, b, generator=gen).to(torch.bfloat16))
    again = _quiet(sdnq_amd.add_lora, m, rank=16, convs=True)
    assert again.added == 0 and "already" in dict(again.skipped)["conv"]           # not wrapped twice
    # float32 master factors
    m2 = toy_model()
    _quiet(sdnq_amd.add_lora, m2, rank=8, dtype=torch.float32, targets=["conv"], convs=True)
    assert m2.conv.lora_down.dtype == torch.float32 and m2.conv.lora_down.shape == (8, 16, 3, 3) and m2.conv1d.lora_up.shape == (32, 8, 1)


def test_enable_input_grad_interplay_and_remove_lora_restores_the_very_forward():
    m = toy_model()
    inference = {n: getattr(m, n).forward_func for n in QUANTIZED}
    assert _quiet(sdnq_amd.enable_input_grad, m, convs=True) >= 3
    switched = {n: getattr(m, n).forward_func for n in QUANTIZED}
    assert switched["conv"] is not inference["conv"]
    assert _quiet(sdnq_amd.add_lora, m, rank=8, convs=True) == 3
    # the adapter wraps the inference forward (its own backward computes the input gradient) ...
    assert m.conv.forward_func._sdnq_lora_base is inference["conv"] and m.conv1d.forward_func._sdnq_lora_base is inference["conv1d"]
    # ... and enable_input_grad called afterwards leaves these layers alone
    res = _quiet(sdnq_amd.enable_input_grad, m, convs=True)
    assert "does not run on the MI355X forwards" in dict(res.skipped)["conv"]
    assert sdnq_amd.remove_lora(m) == 3
    assert all(getattr(m, n).forward_func is switched[n] for n in QUANTIZED)       # the very objects they had before
    for name in ("conv", "conv1d"):
        mod = getattr(m, name)
        assert not any(hasattr(mod, a) for a in ("lora_down", "lora_up", "lora_scale"))
        assert not any("lora" in k for k, _ in mod.named_parameters())
    assert sdnq_amd.remove_lora(m) == 0 and sdnq_amd.lora_state_dict(m) == {}


def test_state_dict_round_trips_under_the_peft_names_with_conv_shapes():
    m = toy_model()
    _quiet(sdnq_amd.add_lora, m, rank=8, seed=1, convs=True)
    with torch.no_grad():
        m.conv.lora_up.copy_(torch.randn(32, 8, 1, 1))
        m.conv1d.lora_up.copy_(torch.randn(32, 8, 1))
    sd = sdnq_amd.lora_state_dict(m)
    assert set(sd) == {f"{n}.lora_{ab}.weight" for n in ("q", "conv", "conv1d") for ab in "AB"}
    assert sd["conv.lora_A.weight"].shape == (8, 16, 3, 3) and sd["conv.lora_B.weight"].shape == (32, 8, 1, 1)
    assert sd["conv1d.lora_A.weight"].shape == (8, 16, 5) and sd["conv1d.lora_B.weight"].shape == (32, 8, 1)
    assert not any(v.requires_grad for v in sd.values())
    # the shapes PEFT itself registers for these layers
    assert sd["conv.lora_A.weight"].shape == torch.nn.Conv2d(16, 8, 3, padding=1, bias=False).weight.shape
    assert sd["conv.lora_B.weight"].shape == torch.nn.Conv2d(8, 32, 1, bias=False).weight.shape
    other = toy_model()
    _quiet(sdnq_amd.add_lora, other, rank=8, seed=2, convs=True)
    peft = {"base_model.model." + k.replace(".weight", ".default.weight"): v.clone() for k, v in sd.items()}
    assert sdnq_amd.load_lora_state_dict(other, peft) == 3
    for name in ("q", "conv", "conv1d"):
        assert torch.equal(getattr(other, name).lora_down, getattr(m, name).lora_down)
        assert torch.equal(getattr(other, name).lora_up, getattr(m, name).lora_up)
    with pytest.raises(ValueError, match="shape"):
        sdnq_amd.load_lora_state_dict(other, {**sd, "conv.lora_A.weight": torch.zeros(8, 144)})


def test_cpu_forward_raises_with_and_without_a_graph():
    m = toy_model()
    _quiet(sdnq_amd.add_lora, m, rank=8, convs=True)
    for mod, x in ((m.conv, torch.randn(2, 16, 8, 8, dtype=torch.bfloat16)), (m.conv1d, torch.randn(2, 16, 40, dtype=torch.bfloat16))):
        with pytest.raises(_lib.SdnqHipError, match="CPU"):
            mod(x)                                 # the factors require grad: QuantizedConvLoRA
        with pytest.raises(_lib.SdnqHipError, match="CPU"):
            with torch.no_grad():
                mod(x)                             # adapter inference
    assert T.scratch_bytes.__module__ == "sdnq_amd.training"
