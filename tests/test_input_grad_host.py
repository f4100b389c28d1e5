"""Input gradients through frozen quantized Linear layers, host side: the two new exports and their argument checks, the import-name
drop-in, and sdnq_amd.enable_input_grad on a model built on the CPU."""
import ctypes
import importlib
import warnings

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, training as T

NEW = ("sdnq_hip_dequant_t", "sdnq_hip_transpose2d")


def test_both_symbols_are_exported_and_bound():
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    arity = {"sdnq_hip_dequant_t": 4, "sdnq_hip_transpose2d": 7}
    for name in NEW:
        assert name in _lib.EXPORTS, name
        fn = getattr(raw, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity[name], name
    assert "dequant_t" in [u[0] for u in importlib.import_module("sdnq_amd._build").UNITS]


def test_argument_validation_without_gpu():
    """Validation runs before any launch, so the status codes are observable without a device."""
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def weight(**kw):
        d = dict(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=40, k=48, group_size=48, svd_rank=0, svd_dtype=0,
                 storage=_lib.ST_RAW8, kind=_lib.KIND_INT, bits=8, exponent=0, mantissa=0, native_float=0, positions=1, scale_dtype=0)
        d.update(kw)
        return ctypes.byref(_lib.SdnqWeight(**d))
    dq = raw.sdnq_hip_dequant_t
    unsupported = _lib.ERR_UNSUPPORTED
    assert unsupported == -5
    assert dq(None, p, 1, None) == -1 and dq(weight(), None, 1, None) == -1 and dq(weight(weight=None), p, 1, None) == -1   # NULL
    assert dq(weight(kind=_lib.KIND_UINT), p, 1, None) == -1                         # unsigned codes without a zero point
    assert dq(weight(), p, 7, None) == -2 and dq(weight(), p, -1, None) == -2        # out dtype
    assert dq(weight(bits=4), p, 1, None) == -2                                      # raw 8-bit storage of 4-bit codes
    assert dq(weight(k=40, group_size=40), p, 1, None) == unsupported                # K % 16
    assert dq(weight(n=36), p, 1, None) == unsupported                               # N % 8
    assert dq(weight(svd_up=p, svd_down=p, svd_rank=8, svd_dtype=1), p, 1, None) == unsupported
    assert dq(weight(group_size=36), p, 1, None) == -3                               # groups do not divide K
    assert dq(weight(), p + 4, 1, None) == -4 and dq(weight(weight=p + 8), p, 1, None) == -4   # misaligned pointers
    tr = raw.sdnq_hip_transpose2d
    ok = dict(x=p, dt=1, r=40, c=48, ldx=48, out=p, stream=None)

    def rc(**broken):
        return tr(*{**ok, **broken}.values())
    assert rc(x=None) == -1 and rc(out=None) == -1
    assert rc(dt=3) == -2 and rc(dt=-1) == -2
    assert rc(ldx=40) == -3                                                          # ldx < c
    assert rc(r=36) == -3 and rc(c=44, ldx=44) == -3 and rc(r=0) == -3               # r % 8, c % 8
    assert rc(x=p + 2) == -4 and rc(out=p + 8) == -4                                 # misaligned pointers
    assert rc(ldx=52) == -4                                                          # bf16 rows of 104 bytes


def test_import_name_drop_in():
    fwd = importlib.import_module("sdnq.training.layers.linear.forward")
    assert fwd.quantized_linear_input_grad is T.quantized_linear_input_grad
    assert fwd.QuantizedLinearInputGrad is T.QuantizedLinearInputGrad
    assert issubclass(T.QuantizedLinearInputGrad, torch.autograd.Function)
    assert sdnq_amd.enable_input_grad is T.enable_input_grad
    doc = fwd.__doc__
    assert "SDNQTensor" in doc and "grad_weight" in doc


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(64, 64)
        self.a = torch.nn.Linear(64, 64)          # stays float: the adapter
        self.q = torch.nn.Linear(64, 48)
        self.odd = torch.nn.Linear(64, 44)        # N % 8 != 0
        self.conv = torch.nn.Conv2d(16, 32, 3, padding=1)

    def forward(self, x):
        return self.q(self.a(x))


def toy_model():
    torch.manual_seed(0)
    m = Toy().to(torch.bfloat16)
    cfg = dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    for name, extra in (("q", {}), ("odd", {}), ("conv", {"quant_conv": True}), ("emb", {"quant_embedding": True})):
        layer, _ = sdnq_amd.sdnq_quantize_layer(getattr(m, name), sdnq_amd.SDNQConfig(**cfg, **extra))
        setattr(m, name, layer)
    assert all(getattr(getattr(m, n), "sdnq_dequantizer", None) is not None for n in ("q", "odd", "conv", "emb"))
    return m


def test_enable_input_grad_wraps_skips_and_restores():
    m = toy_model()
    before = {n: getattr(m, n).forward_func for n in ("q", "odd", "conv", "emb")}
    with pytest.warns(UserWarning, match="still cut the autograd graph") as rec:
        res = sdnq_amd.enable_input_grad(m)
    assert len(rec) == 1
    assert res == 1 and res.enabled == 1 and isinstance(res, int)
    n, skipped = res
    assert n == 1 and skipped == res.skipped
    why = dict(res.skipped)
    assert set(why) == {"odd", "conv", "emb"}
    assert "Linear layers" in why["conv"] and "Conv2d" in why["conv"]
    assert "Linear layers" in why["emb"] and "Embedding" in why["emb"]
    assert "8 | N" in why["odd"] and "N = 44" in why["odd"]
    assert m.q.forward_func is not before["q"] and m.q.forward_func._sdnq_inference_forward is before["q"]
    assert all(getattr(m, k).forward_func is before[k] for k in ("odd", "conv", "emb"))
    assert str(m.q.forward_func.__module__).startswith("sdnq_amd")   # apply_sdnq_options_to_model still sees one of its own forwards
    wrapped = m.q.forward_func
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert sdnq_amd.enable_input_grad(m) == 1 and m.q.forward_func is wrapped       # not wrapped twice
    off = sdnq_amd.enable_input_grad(m, enabled=False)
    assert off == 1 and off.skipped == []
    assert all(getattr(m, k).forward_func is before[k] for k in before)
    assert sdnq_amd.enable_input_grad(m, enabled=False) == 0


def test_layer_dtype_outside_the_floats_is_skipped():
    m = toy_model()
    m.q.sdnq_dequantizer.result_dtype = torch.float64
    with pytest.warns(UserWarning):
        res = sdnq_amd.enable_input_grad(m)
    assert res.enabled == 0 and "float64" in dict(res.skipped)["q"]


def test_cpu_tensors_under_grad_raise():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.enable_input_grad(m)
    x = torch.randn(40, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        m(x)                                      # a.weight requires grad: the quantized layer's input does, too
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        T.quantized_linear_input_grad(m.q, x.requires_grad_())
    # a backward handed a gradient of another dtype names both
    ctx = type("Ctx", (), {"layer": m.q, "input_shape": x.shape, "needs_input_grad": (False, True, False), "bias_dtype": None})()
    with pytest.raises(NotImplementedError, match=r"float32.*bfloat16"):
        T.QuantizedLinearInputGrad.backward(ctx, torch.zeros(40, 48))
