"""Merging adapters into the stored codes, host side: the statuses of sdnq_hip_merge_lowrank (validation runs before any launch, so they
are observable without a device) and the argument checks, key parsing, rank padding and skip sentences of merge_lora /
merge_lora_state_dict on a model built on the CPU (the kernel route of one layer is replaced by a stand-in that records its arguments)."""
import ctypes
import importlib
import warnings

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, lora, ops
from tests.test_lora_host import toy_model


def _raw():
    lib = _lib.load()
    return getattr(lib, "_ctypes", lib)


def test_the_symbol_is_declared_exported_and_built_after_dora():
    fn = _raw().sdnq_hip_merge_lowrank
    assert "sdnq_hip_merge_lowrank" in _lib.EXPORTS and len(fn.argtypes) == 11
    units = [u[0] for u in importlib.import_module("sdnq_amd._build").UNITS]
    assert units.index("merge") == units.index("dora") + 1
    assert sdnq_amd.merge_lora is lora.merge_lora and sdnq_amd.merge_lora_state_dict is lora.merge_lora_state_dict
    assert {"merge_lora", "merge_lora_state_dict"} <= set(sdnq_amd.__all__)


def test_statuses_without_gpu():
    """Every call below fails a check, so nothing is launched: NULL -1, DTYPE -2, SHAPE -3, ALIGN -4, UNSUPPORTED -5."""
    merge = _raw().sdnq_hip_merge_lowrank
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    at = lambda i: p + 4096 * i  # noqa: E731  (regions that do not overlap)

    def desc(base, **kw):
        f = dict(weight=at(base), scale=at(base + 1), n=8, k=16, group_size=16, storage=_lib.ST_RAW8, kind=_lib.KIND_INT, bits=8)
        f.update(kw)
        return _lib.SdnqWeight(**f)

    def rc(w=None, out=None, **kw):
        a = dict(up=at(6), down=at(7), dt=_lib.BF16, rank=8, scale=0.5, row_scale=None, qmin=-128.0, qmax=127.0, stream=None)
        a.update(kw)
        w = desc(0) if w is None else w
        out = desc(3) if out is None else out
        return merge(None if w is False else ctypes.byref(w), None if out is False else ctypes.byref(out), *a.values())

    bad_range = dict(qmin=1.0, qmax=1.0)  # a SHAPE fault checked after the NULL rules: shows that a combination passed them
    # NULL combinations
    assert rc(w=False) == -1 and rc(out=False) == -1
    assert rc(w=desc(0, weight=None)) == -1 and rc(w=desc(0, scale=None)) == -1
    assert rc(out=desc(3, weight=None)) == -1 and rc(out=desc(3, scale=None)) == -1
    assert rc(up=None) == -1 and rc(down=None) == -1                                  # one factor without the other
    assert rc(up=None, down=None) == -1                                               # nothing to merge
    assert rc(up=None, down=None, row_scale=at(8), **bad_range) == -3                 # the pure row rescale passes the NULL rules
    assert rc(row_scale=at(8), **bad_range) == -3
    u8 = dict(kind=_lib.KIND_UINT)
    assert rc(w=desc(0, zero_point=at(2), **u8), out=desc(3, **u8)) == -1             # unsigned: the output needs a zero point
    assert rc(w=desc(0, zero_point=at(2), **u8), out=desc(3, zero_point=at(5), **u8), **bad_range) == -3
    # aliasing of any output with an input or another output
    assert rc(out=desc(0)) == -3 and rc(out=desc(3, weight=at(0) + 64)) == -3         # the codes in place, or overlapping in part
    assert rc(out=desc(3, scale=at(1))) == -3 and rc(out=desc(3, scale=at(6))) == -3  # the scales over w's, over up
    assert rc(out=desc(3, weight=at(7))) == -3 and rc(out=desc(3, scale=at(3))) == -3  # the codes over down; the scales over the codes
    assert rc(row_scale=at(4), out=desc(3, scale=at(4))) == -3
    assert rc(w=desc(0, zero_point=at(2), **u8), out=desc(3, zero_point=at(4), scale=at(4), **u8)) == -3
    # shapes, ranks, alignment, dtypes
    assert rc(w=desc(0, k=24, group_size=24), out=desc(3, k=24, group_size=24)) == -3
    assert rc(w=desc(0, n=12), out=desc(3, n=12)) == -3
    assert rc(rank=12) == -3 and rc(rank=264) == -3 and rc(rank=0) == -3
    assert rc(out=desc(3, n=16)) == -3 and rc(out=desc(3, group_size=8)) == -3
    assert rc(out=desc(3, kind=_lib.KIND_UINT, zero_point=at(5))) == -2 and rc(dt=_lib.F32) == -2
    assert rc(up=at(6) + 8) == -4 and rc(down=at(7) + 2) == -4 and rc(row_scale=at(8) + 2) == -4
    assert rc(out=desc(3, weight=at(3) + 8)) == -4 and rc(out=desc(3, scale=at(4) + 2)) == -4 and rc(w=desc(0, weight=at(0) + 8)) == -4
    # what the kernel is not built for: before any launch, for the caller's composition route
    assert rc(w=desc(0, k=96, group_size=48), out=desc(3, k=96, group_size=48)) == _lib.ERR_UNSUPPORTED
    assert rc(w=desc(0, k=1024, group_size=512), out=desc(3, k=1024, group_size=512)) == _lib.ERR_UNSUPPORTED
    cb = dict(kind=_lib.KIND_CODEBOOK, bits=4, storage=_lib.ST_PACKED_U8)
    assert rc(w=desc(0, **cb), out=desc(3, **cb)) == _lib.ERR_UNSUPPORTED
    pos = dict(k=48, group_size=16, positions=3)
    assert rc(w=desc(0, **pos), out=desc(3, **pos)) == _lib.ERR_UNSUPPORTED
    svd = desc(0, svd_up=at(9), svd_down=at(10), svd_rank=8, svd_dtype=_lib.BF16)       # SVD factors are allowed and ignored
    assert rc(w=svd, **bad_range) == -3


def test_ops_checks_and_the_supported_predicate():
    err = _lib.SdnqHipError
    w = torch.zeros((8, 32), dtype=torch.int8)
    d = _lib.SdnqWeight(weight=1, scale=1, n=8, k=32, group_size=32, storage=_lib.ST_RAW8, kind=_lib.KIND_INT, bits=8)
    qw = ops.QuantWeight(desc=d, n=8, k=32, group_size=32, keep=(w, None, None, None, None))
    assert ops.merge_lowrank_supported(qw) and ops._format_name(d) == "int8"
    for gs, ok in ((16, True), (48, False), (256, True), (512, False)):
        assert ops.merge_lowrank_supported(ops.QuantWeight(desc=d, n=8, k=1536, group_size=gs, keep=(w,))) is ok
    up, down = torch.zeros((8, 8), dtype=torch.bfloat16), torch.zeros((8, 32), dtype=torch.bfloat16)
    with pytest.raises(err, match="nothing to merge"):
        ops.merge_lowrank(qw, None, None)
    with pytest.raises(err, match="both or neither"):
        ops.merge_lowrank(qw, up, None)
    with pytest.raises(err, match=r"up \[N, R\]"):
        ops.merge_lowrank(qw, up, down[:, :16].contiguous())
    with pytest.raises(err, match="not the format"):
        ops.merge_lowrank(qw, up, down, weights_dtype="uint4")
    with pytest.raises(err, match="CPU"):
        ops.merge_lowrank(qw, up, down)
    with pytest.raises(err, match="row_scale"):
        ops.merge_lowrank(qw, up, down, 1.0, torch.zeros(8, dtype=torch.bfloat16))


@pytest.fixture
def recorded(monkeypatch):
    """_merge_layer needs a device: the stand-in records what it was given and reports the fused route."""
    calls = []

    def stand_in(module, down, up, scale, c):
        calls.append((module, down, up, scale, c))
        return "fused"
    monkeypatch.setattr(lora, "_merge_layer", stand_in)
    return calls


def test_merge_lora_merges_skips_and_warns_once(recorded):
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert sdnq_amd.add_lora(m, rank=8, alpha=16, seed=3, convs=True, dtype=torch.float32) == 3
    conv_fwd, conv_weight, conv_down = m.conv.forward_func, m.conv.weight, m.conv.lora_down
    with pytest.warns(UserWarning, match="were not merged") as rec:
        res = sdnq_amd.merge_lora(m)
    assert len(rec) == 1 and isinstance(res, int) and res == 2 and res.merged == ["q", "k"]
    why = dict(res.skipped)
    assert set(why) == {"conv"} and "merging conv adapters is not built" in why["conv"] and "Conv2d" in why["conv"]
    assert m.conv.forward_func is conv_fwd and m.conv.weight is conv_weight and m.conv.lora_down is conv_down   # untouched, adapter on
    assert [c[0] for c in recorded] == [m.q, m.k]
    _, down, up, scale, c = recorded[0]
    assert down.dtype == torch.bfloat16 and up.dtype == torch.bfloat16 and down.shape == (8, 64) and up.shape == (48, 8)   # the layer dtype
    assert scale == 2.0 and c is None and down.is_contiguous() and up.is_contiguous()
    for mod in (m.q, m.k):                                                                                       # as remove_lora leaves them
        assert not any(hasattr(mod, a) for a in ("lora_down", "lora_up", "lora_scale", "lora_dropout"))
        assert mod.forward_func.__module__ != "sdnq_amd.lora"
    assert sdnq_amd.merge_lora(m, targets=["q"]) == 0                                                            # nothing selected is left


def test_merge_lora_targets(recorded):
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, seed=3)
    res = sdnq_amd.merge_lora(m, targets=["k"])
    assert res == 1 and res.merged == ["k"] and res.skipped == [] and hasattr(m.q, "lora_down") and not hasattr(m.k, "lora_down")


def test_dora_on_svd_factors_has_its_sentence():
    m = toy_model()
    assert lora.merge_unsupported_reason(m.q, dora=True) is None
    m.q.svd_up = torch.zeros(48, 8)
    assert lora.merge_unsupported_reason(m.q, dora=False) is None
    why = lora.merge_unsupported_reason(m.q, dora=True)
    assert "DoRA" in why and "SVD" in why and "not built" in why


def test_state_dict_keys_rank_padding_and_scale(recorded):
    m = toy_model()
    a, b = torch.randn(4, 64), torch.randn(48, 4)
    a2, b2 = torch.randn(16, 64), torch.randn(72, 16)
    sd = {"base_model.model.q.lora_A.default.weight": a, "base_model.model.q.lora_B.default.weight": b,
          "k.lora_A.weight": a2, "k.lora_B.weight": b2}
    res = sdnq_amd.merge_lora_state_dict(m, sd, scale=0.25)
    assert res == 2 and res.merged == ["q", "k"] and res.skipped == []
    (mq, down, up, scale, c), (mk, down2, up2, scale2, _) = recorded
    assert mq is m.q and mk is m.k and scale == 0.25 and scale2 == 0.25 and c is None
    assert down.shape == (8, 64) and up.shape == (48, 8) and down.dtype == torch.bfloat16 and down.is_contiguous() and up.is_contiguous()
    assert torch.equal(down[:4], a.to(torch.bfloat16)) and not bool(down[4:].any())          # zero rows of down ...
    assert torch.equal(up[:, :4], b.to(torch.bfloat16)) and not bool(up[:, 4:].any())        # ... and zero columns of up
    assert down2.shape == (16, 64) and torch.equal(down2, a2.to(torch.bfloat16))             # a multiple of 8 is left as it is
    d12, u12 = lora.pad_rank(torch.ones(12, 16), torch.ones(8, 12))
    assert d12.shape == (16, 16) and u12.shape == (8, 16) and float(d12.sum()) == 12 * 16 and float(u12.sum()) == 8 * 12
    assert not any(hasattr(m.q, x) for x in ("lora_down", "lora_up", "lora_scale"))          # no adapter is put on


def test_state_dict_argument_checks_touch_nothing(recorded):
    m = toy_model()
    a, b = torch.randn(8, 64), torch.randn(48, 8)
    good = {"q.lora_A.weight": a, "q.lora_B.weight": b}
    with pytest.raises(KeyError, match="not a <module>"):
        sdnq_amd.merge_lora_state_dict(m, {**good, "q.weight": a})
    with pytest.raises(KeyError, match="no quantized layer"):
        sdnq_amd.merge_lora_state_dict(m, {**good, "nosuch.lora_A.weight": a, "nosuch.lora_B.weight": b})
    with pytest.raises(KeyError, match="no quantized layer"):                                  # `a` stays float: not an SDNQ layer
        sdnq_amd.merge_lora_state_dict(m, {"a.lora_A.weight": a, "a.lora_B.weight": torch.randn(64, 8)})
    with pytest.raises(KeyError, match="needs both"):
        sdnq_amd.merge_lora_state_dict(m, {**good, "k.lora_A.weight": a})
    with pytest.raises(ValueError, match=r"lora_A \[r, 64\]"):
        sdnq_amd.merge_lora_state_dict(m, {**good, "k.lora_A.weight": a, "k.lora_B.weight": b})   # k has 72 rows
    with pytest.raises(ValueError, match="lora_magnitude_vector"):
        sdnq_amd.merge_lora_state_dict(m, {**good, "q.lora_magnitude_vector.weight": torch.ones(40)})
    with pytest.raises(ValueError, match="finite"):
        sdnq_amd.merge_lora_state_dict(m, good, scale=float("nan"))
    assert recorded == []                                                                      # every check came before the first merge
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, targets=["q"])
    with pytest.raises(ValueError, match="carries an adapter"):
        sdnq_amd.merge_lora_state_dict(m, good)
    assert recorded == [] and hasattr(m.q, "lora_down")


def test_state_dict_skips_with_sentences_and_one_warning(recorded):
    m = toy_model()
    before = {n: (getattr(m, n).weight, getattr(m, n).scale, getattr(m, n).forward_func) for n in ("conv", "f32", "odd")}
    sd = {"q.lora_A.weight": torch.randn(8, 64), "q.lora_B.weight": torch.randn(48, 8),
          "conv.lora_A.weight": torch.randn(8, 16, 3, 3), "conv.lora_B.weight": torch.randn(32, 8, 1, 1),
          "f32.lora_A.weight": torch.randn(8, 64), "f32.lora_B.weight": torch.randn(48, 8),
          "odd.lora_A.weight": torch.randn(8, 64), "odd.lora_B.weight": torch.randn(44, 8)}
    with pytest.warns(UserWarning, match="were not merged") as rec:
        res = sdnq_amd.merge_lora_state_dict(m, sd)
    assert len(rec) == 1 and res == 1 and res.merged == ["q"]
    why = dict(res.skipped)
    assert set(why) == {"conv", "f32", "odd"}
    assert "merging conv adapters is not built" in why["conv"] and "float32" in why["f32"] and "8 | N" in why["odd"]
    assert all(n in str(rec[0].message) for n in why)
    for n, (w, s, f) in before.items():
        mod = getattr(m, n)
        assert mod.weight is w and mod.scale is s and mod.forward_func is f and not hasattr(mod, "lora_down")
    assert [c[0] for c in recorded] == [m.q]
