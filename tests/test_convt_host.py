"""Transposed convolutions, host side (no GPU): the quantizer against the reference's stored tensors, the forward dispatch, the support
predicate, the wrapper classes, the loader on a reference-written checkpoint, and the C ABI of the new entry points."""
import ctypes
import json
import os

import pytest
import torch

from tests import convt_util as U
from tests.header_util import declared_arity


@pytest.mark.parametrize("name", U.NAMES)
def test_host_quantizer_reproduces_the_reference(name):
    """sdnq_quantize_layer on the fixture's float layer: stored tensors bit for bit, every dequantizer field, the wrapper class and the
    forward the reference picked."""
    meta, t = U.load(name)
    q = U.quantize_here(meta, t)
    assert U.deq_fields(q.sdnq_dequantizer) == meta["deq"]
    assert q.sdnq_dequantizer.use_quantized_matmul is False
    for key in ("weight", "scale", "zero_point"):
        mine = getattr(q, key)
        if key not in t:
            assert mine is None, key
            continue
        assert mine.dtype == t[key].dtype and tuple(mine.shape) == tuple(t[key].shape), (key, mine.dtype, mine.shape)
        assert torch.equal(U.bits(mine), U.bits(t[key])), key
    assert type(q).__name__ == f"SDNQConvTranspose{meta['nd']}d" and q.forward_func.__name__ == meta["forward_func"]
    assert q.forward_func.__module__ == "sdnq_amd.conv_transpose"


@pytest.mark.parametrize("shape, cfg", [((64, 32, 4, 4), dict(weights_dtype="uint4")), ((64, 48, 16), dict(weights_dtype="uint4")),
                                        ((64, 32, 4, 4), dict(weights_dtype="int8", group_size=16))])
def test_non_square_grouped_layout_raises_by_name(shape, cfg):
    """Group quantization of a weight with C_out / groups != C_in: the reference's own unflatten fails; here NotImplementedError that says so
    and names group_size=-1."""
    import sdnq_amd
    w = torch.randn(shape)
    with pytest.raises(NotImplementedError, match=r"C_out / groups == C_in.*group_size=-1"):
        sdnq_amd.sdnq_quantize_layer_weight(w, layer_class_name=f"ConvTranspose{len(shape) - 2}d", **cfg)
    dq, data = sdnq_amd.sdnq_quantize_layer_weight(w, layer_class_name=f"ConvTranspose{len(shape) - 2}d", **dict(cfg, group_size=-1))
    assert dq.group_size == -1 and tuple(data["scale"].shape) == (1, *shape[1:])


def test_size_rule_reads_the_input_channels():
    """minimum_allowed_channel_size applies to weight.shape[0] of a transposed conv (utils.py:84-85), and quant_conv gates the class."""
    import sdnq_amd

    def net(c_in, c_out):
        return torch.nn.Sequential(torch.nn.ConvTranspose2d(c_in, c_out, 4))
    cfg = dict(weights_dtype="int8", minimum_allowed_numel=1024)
    m = sdnq_amd.sdnq_post_load_quant(net(16, 64), quantization_config=sdnq_amd.SDNQConfig(quant_conv=True, **cfg))
    assert type(m[0]) is torch.nn.ConvTranspose2d  # C_in = 16 < 32
    m = sdnq_amd.sdnq_post_load_quant(net(64, 16), quantization_config=sdnq_amd.SDNQConfig(quant_conv=True, **cfg))
    assert type(m[0]).__name__ == "SDNQConvTranspose2d"
    m = sdnq_amd.sdnq_post_load_quant(net(64, 16), quantization_config=sdnq_amd.SDNQConfig(quant_conv=False, **cfg))
    assert type(m[0]) is torch.nn.ConvTranspose2d


def test_get_forward_func_returns_the_three_forwards():
    from sdnq_amd import conv_transpose
    from sdnq_amd.forward import get_forward_func
    for nd in (1, 2, 3):
        want = getattr(conv_transpose, f"quantized_conv_transpose_{nd}d_forward")
        for cls in (f"ConvTranspose{nd}d", f"SDNQConvTranspose{nd}d"):
            for qmm in (False, True):  # never a quantized matmul, whatever the config says (quantizer.py:133)
                assert get_forward_func(cls, "int8", qmm) is want
    import inspect
    assert list(inspect.signature(conv_transpose.quantized_conv_transpose_2d_forward).parameters) == ["self", "input", "output_size"]


def test_forward_refuses_cpu_tensors_and_wrong_dtypes():
    from sdnq_amd._lib import SdnqHipError
    meta, t = U.load("2d_int8_bf16")
    mod = U.stored_module(meta, t)
    with pytest.raises(SdnqHipError):
        mod(t["x"])
    with pytest.raises(RuntimeError, match="expected input dtype"):
        mod(t["x"].float())


@pytest.mark.parametrize("name", U.NAMES)
def test_unsupported_reason_is_none_for_the_fixtures(name):
    from sdnq_amd.support import unsupported_reason
    meta, t = U.load(name)
    assert unsupported_reason(U.stored_module(meta, t)) is None


def test_unsupported_reason_names_what_is_not_built():
    from sdnq_amd.support import unsupported_reason
    meta, t = U.load("2d_int8_bf16")
    mod = U.stored_module(meta, t)
    mod.svd_up = torch.nn.Parameter(torch.zeros(64, 8), requires_grad=False)
    mod.svd_down = torch.nn.Parameter(torch.zeros(8, 512), requires_grad=False)
    assert "SVD factors on transposed convolutions" in unsupported_reason(mod)
    mod.svd_up = mod.svd_down = None
    mod.sdnq_dequantizer.use_hadamard = True
    assert "Hadamard rotation on transposed convolutions" in unsupported_reason(mod)
    mod.sdnq_dequantizer.use_hadamard = False
    mod.sdnq_dequantizer.use_codebook = True
    assert "codebooks on transposed convolutions" in unsupported_reason(mod)
    mod.sdnq_dequantizer.use_codebook = False
    mod.padding_mode = "reflect"
    assert "padding modes" in unsupported_reason(mod)
    mod.padding_mode = "zeros"
    assert unsupported_reason(mod) is None
    # the divisibility the kernels need: 16 | C_in / groups, 16 | C_out / groups * prod(kernel)
    mod.groups = 8
    assert "16 | C_in / groups" in unsupported_reason(mod)
    mod.groups = 1
    mod.sdnq_dequantizer.original_shape = torch.Size([64, 3, 3, 3])
    assert "16 | C_out / groups * prod(kernel)" in unsupported_reason(mod)


def test_wrapper_classes_under_both_import_names():
    import sdnq.layers
    import sdnq_amd.layers
    for nd in (1, 2, 3):
        cls = getattr(sdnq_amd.layers, f"SDNQConvTranspose{nd}d")
        assert getattr(sdnq.layers, f"SDNQConvTranspose{nd}d") is cls
        assert issubclass(cls, sdnq_amd.layers.SDNQLayer) and issubclass(cls, getattr(torch.nn, f"ConvTranspose{nd}d"))
    layer = torch.nn.ConvTranspose1d(32, 32, 4)
    assert type(sdnq_amd.layers.get_sdnq_wrapper_class(layer, lambda *a: None)) is sdnq_amd.layers.SDNQConvTranspose1d


@pytest.mark.parametrize("name", ["2d_int8_bf16", "2d_sq_uint4_grouped_f16", "2d_groups2_int8_bf16", "2d_dil_outsize_f16", "1d_fp8_bf16",
                                  "3d_int8_nobias_bf16"])
def test_compile_operator_traces_the_output_shape(name):
    """accelerate() gives a transposed-conv layer the handle of the opaque `sdnq_hip::layer_forward` operator; the operator's fake
    implementation (what torch.compile traces with) must return the shape torch's own ConvTransposeNd gives -- batched and unbatched."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import sdnq_amd
    from sdnq_amd import layers
    meta, t = U.load(name)
    model = torch.nn.Sequential(U.stored_module(meta, t))
    mod = model[0]
    mod.__dict__.pop("_sdnq_hip_handle", None)
    assert sdnq_amd.accelerate(model).accelerated == 1
    handle = mod.__dict__["_sdnq_hip_handle"]
    assert layers._traceable(mod) and mod.__dict__["_sdnq_hip_plan"] is None
    want = U.float_layer(meta, t)(t["x"])  # the module's own output_padding, no output_size=
    with FakeTensorMode() as mode:
        x = mode.from_tensor(t["x"])
        y = torch.ops.sdnq_hip.layer_forward(x, handle)
        assert tuple(y.shape) == tuple(want.shape) and y.dtype == want.dtype
        y1 = torch.ops.sdnq_hip.layer_forward(x[0], handle)
        assert tuple(y1.shape) == tuple(want.shape[1:])
    # a freshly quantized layer traces the same way (SDNQLayer.__init__ assigns the handle)
    fresh = U.quantize_here(meta, t)
    assert "_sdnq_hip_handle" in fresh.__dict__


class TinyUp(torch.nn.Module):
    """The skeleton of tests/golden/convt_checkpoint_tiny (the checkpoint holds only tensors + json)."""

    def __init__(self, c_in=64, c_out=32):
        super().__init__()
        self.proj = torch.nn.Linear(c_in, c_in)
        self.up = torch.nn.ConvTranspose2d(c_in, c_out, 4, stride=2, padding=1)

    def forward(self, x):
        return self.up(self.proj(x.movedim(1, -1)).movedim(-1, 1))


CKPT = os.path.join(U.GOLDEN, "convt_checkpoint_tiny")


def test_reference_checkpoint_loads_and_round_trips(tmp_path):
    """load_sdnq_model rebuilds the transposed-conv layer of a reference-written checkpoint on this package's forward, and
    save_sdnq_model writes the same checkpoint back: every tensor bit for bit under the same key."""
    from safetensors.torch import load_file
    import sdnq_amd
    model = sdnq_amd.load_sdnq_model(CKPT, model_cls=TinyUp, dtype=torch.bfloat16, device="cpu")
    up = model.up
    assert type(up).__name__ == "SDNQConvTranspose2d" and up.forward_func.__module__ == "sdnq_amd.conv_transpose"
    dq = up.sdnq_dequantizer
    assert dq.layer_class_name == "ConvTranspose2d" and dq.use_quantized_matmul is False and dq.group_size == -1
    assert tuple(up.weight.shape) == (64, 32, 4, 4) and up.weight.dtype == torch.int8 and tuple(up.scale.shape) == (1, 32, 4, 4)
    assert not any(p.is_meta for p in model.parameters())
    want = load_file(os.path.join(CKPT, "model.safetensors"))
    sdnq_amd.save_sdnq_model(model, str(tmp_path / "a"))
    got = load_file(str(tmp_path / "a" / "model.safetensors"))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
    cfg, want_cfg = (json.load(open(os.path.join(p, "quantization_config.json"))) for p in (str(tmp_path / "a"), CKPT))
    assert cfg["quant_conv"] is True and cfg["weights_dtype"] == want_cfg["weights_dtype"]
    again = sdnq_amd.load_sdnq_model(str(tmp_path / "a"), model_cls=TinyUp, dtype=torch.bfloat16, device="cpu")
    for (k, a), (_, b) in zip(model.state_dict().items(), again.state_dict().items()):
        assert a.dtype == b.dtype and torch.equal(a, b), k


def test_hf_quantizer_converts_transposed_convs():
    """The HF plugin path: the pre-quantized skeleton of a model with a ConvTranspose2d gets the SDNQ wrapper with placeholders of the
    stored shapes (sdnq_post_load_quant(pre_quantized=True) on the meta device, what SDNQQuantizer runs before the weights are loaded)."""
    import sdnq_amd
    with torch.device("meta"):
        skel = TinyUp()
    cfg = sdnq_amd.SDNQConfig.from_dict(json.load(open(os.path.join(CKPT, "quantization_config.json"))))
    skel = sdnq_amd.sdnq_post_load_quant(skel, torch_dtype=torch.bfloat16, quantization_config=cfg, pre_quantized=True)
    assert type(skel.up).__name__ == "SDNQConvTranspose2d"
    assert tuple(skel.up.weight.shape) == (64, 32, 4, 4) and skel.up.weight.dtype == torch.int8 and tuple(skel.up.scale.shape) == (1, 32, 4, 4)


NEW = ("sdnq_hip_dequant_convt", "sdnq_hip_linear_float_f32out", "sdnq_hip_linear_float_f32out_strided", "sdnq_hip_col2im")


def test_header_prototypes_equal_the_exports():
    """Every new entry point is declared in include/sdnq_hip.h, listed in _lib.EXPORTS, exported by the library, and bound with as many
    ctypes arguments as the prototype has parameters."""
    from sdnq_amd import _lib
    decl = declared_arity()
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    for name in NEW:
        assert name in decl and name in _lib.EXPORTS, name
        fn = getattr(raw, name)
        assert fn.argtypes is not None and len(fn.argtypes) == decl[name], name
    units = [u[0] for u in __import__("sdnq_amd._build", fromlist=["UNITS"]).UNITS]
    assert "convt" in units


def test_argument_validation_without_gpu():
    """Validation runs before any launch, so the status codes are observable without a device."""
    from sdnq_amd import _lib
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    W = _lib.SdnqWeight

    def weight(**kw):
        d = dict(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=64, k=512, group_size=512, svd_rank=0, svd_dtype=0,
                 storage=_lib.ST_RAW8, kind=_lib.KIND_INT, bits=8, exponent=0, mantissa=0, native_float=0, positions=16, scale_dtype=0)
        d.update(kw)
        return W(**d)
    dq = raw.sdnq_hip_dequant_convt
    assert dq(None, 1, 1, p, 1, None) == -1
    assert dq(ctypes.byref(weight()), 1, 1, p, 7, None) == -2                       # out dtype
    assert dq(ctypes.byref(weight(k=520)), 1, 1, p, 1, None) == -3                  # P % 16
    assert dq(ctypes.byref(weight()), 8, 1, p, 1, None) == -3                       # C_in / groups % 16
    assert dq(ctypes.byref(weight()), 1, 5, p, 1, None) == -3                       # scale groups do not divide C_out / groups
    assert dq(ctypes.byref(weight(kind=_lib.KIND_UINT)), 1, 1, p, 1, None) == -1    # unsigned without zero point
    assert dq(ctypes.byref(weight(kind=_lib.KIND_CODEBOOK)), 1, 1, p, 1, None) == -5
    assert dq(ctypes.byref(weight(svd_up=p, svd_down=p, svd_rank=8)), 1, 1, p, 1, None) == -5
    assert dq(ctypes.byref(weight()), 1, 1, p + 4, 1, None) == -4
    f32 = raw.sdnq_hip_linear_float_f32out_strided
    assert f32(None, p, 1, p, 4, 8, 16, 16, 8, None) == -1
    assert f32(p, p, 1, p, 4, 8, 12, 12, 8, None) == -3                             # K * 2 bytes % 16
    assert f32(p, p, 1, p, 4, 8, 16, 16, 4, None) == -3                             # ldc < n
    assert f32(p, p, 1, p + 2, 4, 8, 16, 16, 8, None) == -4
    c2i = raw.sdnq_hip_col2im
    geo = dict(batch=1, channels=2, ind=1, inh=3, inw=3, od=1, oh=6, ow=6, kd=1, kh=2, kw=2, sd=1, sh=2, sw=2, pd=0, ph=0, pw=0, dd=1, dh=1, dw=1)

    def call(cols=p, ld=8, dtype=1, out=p, **kw):
        g = dict(geo, **kw)
        return c2i(cols, ld, None, dtype, out, *g.values(), None)
    assert call(cols=None) == -1
    assert call(dtype=3) == -2
    assert call(ld=7) == -3          # fewer columns than channels * prod(kernel)
    assert call(oh=8) == -3          # beyond output_padding < max(stride, dilation)
    assert call(oh=5) == -3          # below the geometry's own extent
    assert call(sh=0) == -3
    assert call(cols=p + 2) == -4
