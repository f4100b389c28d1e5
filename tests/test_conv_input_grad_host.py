"""Input gradients through frozen quantized Conv1d / Conv2d layers, host side: the switch (enable_input_grad(convs=...)), the predicate's
sentences, the refusals of CPU tensors, the status codes of sdnq_hip_im2col_bwd, and the index maps of the backward-data convolution
(tests/conv_grad_util.py) against torch.nn.grad.conv{1,2}d_input in float64."""
import ctypes
import warnings

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, training as T
from tests import conv_grad_util as U
from tests.golden_util import ConvCase
from tests.test_input_grad_host import toy_model

TODAY = "{}: input gradients are built for quantized Linear layers (conv, transposed-conv and embedding layers are not)"


def test_default_leaves_convs_skipped_with_todays_sentences():
    m = toy_model()
    with pytest.warns(UserWarning, match="still cut the autograd graph"):
        res = sdnq_amd.enable_input_grad(m)
    why = dict(res.skipped)
    assert res.enabled == 1 and set(why) == {"odd", "conv", "emb"}
    assert why["conv"] == TODAY.format(m.conv.sdnq_dequantizer.layer_class_name)
    assert why["emb"] == TODAY.format(m.emb.sdnq_dequantizer.layer_class_name)
    assert why["odd"] == "input gradients need 16 | K and 8 | N (got K = 64, N = 44): the transposed weight leaves in 16-byte runs"
    assert T.input_grad_unsupported_reason(m.conv) == why["conv"] == T.input_grad_unsupported_reason(m.conv, convs=False)
    m2 = toy_model()
    with pytest.warns(UserWarning):
        assert dict(sdnq_amd.enable_input_grad(m2, True, False).skipped) == why          # positional, explicit default


def test_convs_true_wraps_restores_and_is_idempotent():
    m = toy_model()
    before = {n: getattr(m, n).forward_func for n in ("q", "odd", "conv", "emb")}
    assert T.input_grad_unsupported_reason(m.conv, convs=True) is None
    with pytest.warns(UserWarning, match="still cut the autograd graph") as rec:
        res = sdnq_amd.enable_input_grad(m, convs=True)
    assert len(rec) == 1 and res.enabled == 2
    why = dict(res.skipped)
    assert set(why) == {"odd", "emb"}
    assert "Conv1d and Conv2d" in why["emb"] and "Embedding" in why["emb"]
    wrapped = m.conv.forward_func
    assert wrapped is not before["conv"] and wrapped._sdnq_inference_forward is before["conv"]
    assert str(wrapped.__module__).startswith("sdnq_amd") and wrapped.__name__.endswith("_with_input_grad")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert sdnq_amd.enable_input_grad(m, convs=True) == 2 and m.conv.forward_func is wrapped       # not wrapped twice
        assert sdnq_amd.enable_input_grad(m) == 2 and m.conv.forward_func is wrapped                   # a later default call keeps it
    off = sdnq_amd.enable_input_grad(m, enabled=False)
    assert off == 2 and off.skipped == []
    assert all(getattr(m, k).forward_func is before[k] for k in before)
    assert sdnq_amd.enable_input_grad(m, enabled=False, convs=True) == 0


def test_cpu_tensors_under_grad_raise():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.enable_input_grad(m, convs=True)
    x = torch.randn(2, 16, 8, 8, dtype=torch.bfloat16).requires_grad_()
    with pytest.raises(_lib.SdnqHipError, match="conv.*CPU"):
        m.conv(x)
    with pytest.raises(_lib.SdnqHipError, match="conv.*CPU"):
        T.quantized_conv_input_grad(m.conv, x)
    ctx = type("Ctx", (), {"layer": m.conv, "input_shape": x.shape, "needs_input_grad": (False, True, False), "bias_dtype": None})()
    with pytest.raises(NotImplementedError, match=r"float32.*conv.*bfloat16"):
        T.QuantizedConvInputGrad.backward(ctx, torch.zeros(2, 32, 8, 8))
    with pytest.raises(_lib.SdnqHipError, match="conv.*grad_output.*CPU"):
        T.QuantizedConvInputGrad.backward(ctx, torch.zeros(2, 32, 8, 8, dtype=torch.bfloat16))
    assert issubclass(T.QuantizedConvInputGrad, torch.autograd.Function)


def conv_layer(cin, cout, kernel, nd=2, dtype=torch.bfloat16, **kw):
    torch.manual_seed(0)
    ctor = torch.nn.Conv1d if nd == 1 else torch.nn.Conv2d
    layer, _ = sdnq_amd.sdnq_quantize_layer(ctor(cin, cout, kernel, **kw).to(dtype),
                                            sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True, quant_conv=True))
    assert getattr(layer, "sdnq_dequantizer", None) is not None
    return layer


def test_predicate_sentences():
    why = lambda mod: T.input_grad_unsupported_reason(mod, convs=True)  # noqa: E731
    assert why(conv_layer(16, 32, 3, padding=1)) is None
    assert why(conv_layer(16, 32, 3, nd=1, stride=2)) is None
    assert why(conv_layer(32, 32, 3, groups=2)) is None
    # Conv3d, transposed convs, embeddings
    c3 = ConvCase("conv3d_int8_qmm_bf16").torch_module(None)
    assert "Conv3d" in why(c3) and "Conv1d and Conv2d layers" in why(c3)
    m = toy_model()
    assert "Embedding" in why(m.emb) and "embedding layers are not" in why(m.emb)
    ct, _ = sdnq_amd.sdnq_quantize_layer(torch.nn.ConvTranspose2d(32, 32, 2).to(torch.bfloat16),
                                         sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, quant_conv=True))
    assert "ConvTranspose2d" in why(ct) and "transposed-conv" in why(ct)
    # padding
    refl = ConvCase("conv2d_int8_qmm_dil_reflect_bf16").torch_module(None)
    assert "padding_mode='reflect'" in why(refl) and "zero padding" in why(refl)
    same = conv_layer(16, 32, 3, padding="same")
    assert "padding='same'" in why(same)
    # a forward from elsewhere
    foreign = conv_layer(16, 32, 3)
    foreign.forward_func = lambda self, x: x
    assert "sdnq_amd.accelerate(model) first" in why(foreign)
    # what the HIP forwards do not compute says so in support.unsupported_reason's words
    unsup = conv_layer(16, 32, 3)
    unsup.sdnq_dequantizer.use_quantized_matmul, unsup.sdnq_dequantizer.quantized_matmul_dtype = True, "float16"
    from sdnq_amd.support import unsupported_reason
    assert unsupported_reason(unsup) is not None and why(unsup) == unsupported_reason(unsup)
    # the widths dequant_t / transpose2d / linear_float take: 16 | C_in / groups * prod(kernel), 8 | C_out / groups
    odd_k = why(conv_layer(8, 32, 1))
    assert "16 | C_in / groups * prod(kernel)" in odd_k and "(got 8, 32;" in odd_k and "reduction C_out / groups * prod(kernel) = 32" in odd_k
    odd_n = why(conv_layer(16, 24, 3, groups=2))
    assert "8 | C_out / groups" in odd_n and "(got 72, 12;" in odd_n and "width C_in / groups = 8" in odd_n
    # dtype
    f64 = conv_layer(16, 32, 3)
    f64.sdnq_dequantizer.result_dtype = torch.float64
    assert "float64" in why(f64)
    # every one of them lands in .skipped and in the ONE warning
    box = torch.nn.ModuleDict(dict(c3=c3, refl=refl, same=same, foreign=foreign, odd_k=conv_layer(8, 32, 1), f64=f64, ok=conv_layer(16, 32, 3)))
    with pytest.warns(UserWarning, match="6 SDNQ layer") as rec:
        res = sdnq_amd.enable_input_grad(box, convs=True)
    assert len(rec) == 1 and res.enabled == 1 and {n for n, _ in res.skipped} == {"c3", "refl", "same", "foreign", "odd_k", "f64"}


def test_route_rule(monkeypatch):
    """The static rule of section `_takes_col2im_route`: ungrouped layers with a stride, or larger than 1 x 1 on at most 1024 input
    positions, take the transposed-conv kernels; everything else gathers; the switch forces either route for ungrouped layers."""
    rule = T._takes_col2im_route
    assert T.CONV_GRAD_ROUTE is None
    assert rule(1, 9, (2, 2), 16384) and rule(1, 9, (1, 2), 16384) and rule(1, 16, (1, 8), 64)
    assert rule(1, 9, (1, 1), 1024) and not rule(1, 9, (1, 1), 1025) and not rule(1, 9, (1, 1), 16384)
    assert not rule(1, 1, (1, 1), 64) and rule(1, 1, (2, 2), 64)
    assert not rule(2, 9, (2, 2), 64) and not rule(4, 9, (1, 1), 64)
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", "gather")
    assert not rule(1, 9, (2, 2), 64)
    monkeypatch.setattr(T, "CONV_GRAD_ROUTE", "col2im")
    assert rule(1, 1, (1, 1), 10 ** 6) and not rule(2, 9, (2, 2), 64)


def test_im2col_bwd_is_exported_and_validates_without_gpu():
    """Validation runs before any launch, so the status codes are observable without a device."""
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    assert "sdnq_hip_im2col_bwd" in _lib.EXPORTS
    fn = raw.sdnq_hip_im2col_bwd
    assert fn.argtypes is not None and len(fn.argtypes) == 21
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    ok = dict(dy=p, dtype=1, batch=2, channels=24, out_h=8, out_w=8, in_h=16, in_w=16, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, dh=1, dw=1,
              groups=1, row0=0, rows=512, out=p, stream=None)

    def rc(**broken):
        return fn(*{**ok, **broken}.values())
    assert rc(dy=None) == -1 and rc(out=None) == -1                                                   # NULL
    assert rc(dtype=3) == -2 and rc(dtype=-1) == -2                                                   # dtype
    for zero in ("batch", "channels", "out_h", "out_w", "in_h", "in_w", "kh", "kw", "sh", "sw", "dh", "dw", "groups"):
        assert rc(**{zero: 0}) == -3, zero
    assert rc(ph=-1) == -3 and rc(pw=-1) == -3
    assert rc(groups=5) == -3                                                                         # groups do not divide the channels
    assert rc(in_h=17) == -3 and rc(in_h=18) == -3 and rc(out_w=7) == -3                              # extents that do not belong together (17 -> 9 rows)
    assert rc(row0=-1) == -3 and rc(rows=0) == -3 and rc(rows=513) == -3 and rc(row0=1, rows=512) == -3   # the row window
    assert rc(in_h=15) == -3                                                  # 15 rows give 8 output rows as well: now the window is too long
    assert rc(channels=4, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, out_h=16, out_w=16) == -3               # 8-byte rows
    assert rc(channels=2, dtype=0, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, out_h=16, out_w=16) == -3      # float32: 8-byte rows
    assert rc(out=p + 8) == -4                                                                        # misaligned out
    assert rc(channels=64 * 65535 // 9 // 8 * 8 + 8, rows=1) == _lib.ERR_UNSUPPORTED == -5            # the launch grid


@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("geom", U.GEOMETRIES, ids=U.geometry_id)
def test_index_maps_reproduce_the_library_in_float64(geom, groups):
    kernel, stride, padding, dilation, in_hw = U.as_2d(geom)
    ho, wo = U.out_hw(in_hw, kernel, stride, padding, dilation)
    cin = 16
    for cout in U.C_OUTS:
        g = torch.Generator().manual_seed(cout * 10 + groups)
        w = torch.randn(cout, cin // groups, *geom[1], generator=g, dtype=torch.float64)
        dy = torch.randn(U.BATCH, cout, *((wo,) if geom[0] == 1 else (ho, wo)), generator=g, dtype=torch.float64)
        want = U.library_grad_input(geom, dy, w, groups)
        dy4, w4 = (dy.unsqueeze(2), w.unsqueeze(2)) if geom[0] == 1 else (dy, w)
        got = U.grad_input_restated(dy4, w4, in_hw, kernel, stride, padding, dilation, groups)
        got = got.squeeze(2) if geom[0] == 1 else got
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (U.geometry_id(geom), cout, groups)
        u = U.unfold_bwd(dy4, in_hw, kernel, stride, padding, dilation, groups)
        assert u.shape == (U.BATCH * in_hw[0] * in_hw[1], kernel[0] * kernel[1] * cout)
        if groups == 1:   # the column order is (kernel position, channel)
            b, ih, iw, kpos, co = 1, in_hw[0] // 2, in_hw[1] // 2, kernel[0] * kernel[1] - 1, cout - 3
            i, j = divmod(kpos, kernel[1])
            th, tw = ih + padding[0] - i * dilation[0], iw + padding[1] - j * dilation[1]
            hit = th >= 0 and tw >= 0 and th % stride[0] == 0 and tw % stride[1] == 0 and th // stride[0] < ho and tw // stride[1] < wo
            cell = u[(b * in_hw[0] + ih) * in_hw[1] + iw, kpos * cout + co]
            assert cell == (dy4[b, co, th // stride[0], tw // stride[1]] if hit else 0.0)
