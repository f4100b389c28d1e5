"""Host-side checks of the optimizer (sdnq_amd.optim) that need no GPU: the reference's group keys and defaults, what raises, the
import-name views, the state-dict round trip, the argument checks of the two entry points, and the float64 restatement of
tests/optim_util.py against the reference's fixtures (tests/golden/optim_adamw_*)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as U  # noqa: E402

from sdnq_amd import _lib, optim  # noqa: E402


def _param(shape=(4, 64), dtype=torch.float32):
    return torch.nn.Parameter(torch.zeros(shape, dtype=dtype))


def test_group_defaults_and_keys_equal_the_reference():
    rec = U.recorded_defaults()
    got = optim.SDNQOptimizer.apply_group_defaults({})
    assert list(got) == list(rec["defaults"])  # the same keys in the same order
    for key, value in rec["defaults"].items():
        assert (list(got[key]) if isinstance(got[key], tuple) else got[key]) == value, key
    assert sorted(optim.AdamW._group_keys) == rec["group_keys"]
    opt = optim.AdamW([_param()], lr=3e-4)
    group = opt.param_groups[0]
    assert set(group) == set(rec["group_keys"]) and group["lr"] == 3e-4 and group["betas"] == (0.9, 0.999)


def test_constructor_forms():
    a, b = _param(), _param((64,))
    for params in ([a, b], (a, b), iter([a, b]), a):
        opt = optim.AdamW(params, weight_decay=0.5)
        assert opt.param_groups[0]["weight_decay"] == 0.5 and opt.param_groups[0]["params"][0] is a
    opt = optim.AdamW([dict(params=[a], lr=1.0), dict(params=[b])], lr=2.0, betas=(0.5, 0.6))
    assert [g["lr"] for g in opt.param_groups] == [1.0, 2.0] and all(g["betas"] == (0.5, 0.6) for g in opt.param_groups)
    t = torch.zeros(4, 64, requires_grad=True)  # a leaf tensor that is no nn.Parameter, as torch.optim takes it
    assert optim.AdamW([t, b], lr=0.5).param_groups[0]["params"][0] is t
    with pytest.raises(ValueError, match="no_such_option"):
        optim.AdamW([a], no_such_option=1)


RAISES = [
    ("use_kahan", dict(use_kahan=True)),
    ("use_cautious", dict(use_cautious=True)),
    ("offload_buffers", dict(offload_buffers=True)),
    ("quantized_buffers_use_svd", dict(use_quantized_buffers=True, quantized_buffers_use_svd=True)),
    ("quantized_buffers_use_hadamard", dict(use_quantized_buffers=True, quantized_buffers_use_hadamard=True)),
    ("quantized_buffers_use_codebook", dict(use_quantized_buffers=True, quantized_buffers_use_codebook=True)),
    ("quantized_buffers_dtype", dict(use_quantized_buffers=True, quantized_buffers_dtype="int8")),
    ("quantized_buffers_dtype", dict(use_quantized_buffers=True, quantized_buffers_dtype="uint4")),
    ("quantized_buffers_group_size", dict(use_quantized_buffers=True, quantized_buffers_group_size=64)),
    ("quantized_buffers_group_size", dict(use_quantized_buffers=True, quantized_buffers_group_size=-1)),
] + [("final_norm_mode='%s'" % m, dict(final_norm_mode=m)) for m in ("rms", "rms_clip", "relative", "rms_scaled", "rms_clip_scaled", "muon")]


@pytest.mark.parametrize("name,kwargs", RAISES, ids=[f"{n}-{i}" for i, (n, _) in enumerate(RAISES)])
def test_unbuilt_options_raise_by_name(name, kwargs):
    with pytest.raises(NotImplementedError, match=name):
        optim.AdamW([_param()], **kwargs)
    # ... and when the option is switched on in a group of a live optimizer
    opt = optim.AdamW([_param()])
    opt.param_groups[0].update(kwargs)
    opt.param_groups[0]["params"][0].grad = torch.zeros(4, 64)
    with pytest.raises(NotImplementedError, match=name):
        opt.step()


def test_unbuilt_parameters_raise():
    class SDNQTensor(torch.Tensor):  # what training.py recognises as the reference's quantized weight: by name
        pass
    with pytest.raises(NotImplementedError, match="SDNQTensor"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, 64).as_subclass(SDNQTensor))])
    # the reference would quantize [512, 48] (>= 16384 elements, 2-D) with a group size it searches for: not built
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        optim.AdamW([_param((512, 48))], use_quantized_buffers=True)
    optim.AdamW([_param((512, 48))])                                      # dense state: any shape
    optim.AdamW([_param((100, 48))], use_quantized_buffers=True)         # below minimum_numel: dense state
    optim.AdamW([_param((512 * 48,))], use_quantized_buffers=True)       # below minimum_ndim: dense state
    with pytest.raises(NotImplementedError, match="float64"):
        optim.AdamW([_param(dtype=torch.float64)])


@pytest.mark.parametrize("name", ["Adafactor", "CAME", "Lion", "Muon"])
def test_other_optimizers_import_and_raise_by_name(name):
    import sdnq.optim
    cls = getattr(sdnq.optim, name)
    assert cls is getattr(optim, name) and name in optim.NOT_BUILT
    with pytest.raises(NotImplementedError, match=name):
        cls([_param()], lr=1e-3)


def test_cpu_parameters_raise_sdnq_hip_error():
    p = _param()
    opt = optim.AdamW([p])
    assert opt.step() is None  # no gradient: nothing to do, as in the reference
    p.grad = torch.ones_like(p)
    with pytest.raises(_lib.SdnqHipError, match="no CPU path"):
        opt.step()
    assert opt.step.__self__ is opt and len(opt.state[p]) == 0


def test_import_name_views_are_the_same_objects():
    import sdnq.optim
    import sdnq.optim.adamw
    import sdnq.optim.optimizer
    import sdnq.optim.utils
    assert sdnq.optim.AdamW is optim.AdamW is sdnq.optim.adamw.AdamW
    assert sdnq.optim.SDNQOptimizer is optim.SDNQOptimizer is sdnq.optim.optimizer.SDNQOptimizer is sdnq.optim.adamw.SDNQOptimizer
    assert sdnq.optim.utils.QuantizedBuffer is optim.QuantizedBuffer
    assert sdnq.optim.__all__ == ["SDNQOptimizer", "Adafactor", "AdamW", "CAME", "Lion", "Muon"]
    assert issubclass(optim.AdamW, optim.SDNQOptimizer) and issubclass(optim.SDNQOptimizer, torch.optim.Optimizer)


def test_quantized_buffer_layout_and_dequantize():
    qb = optim.QuantizedBuffer.zeros((6, 160), "cpu")
    assert qb.weight.shape == (6, 5, 32) and qb.weight.dtype == torch.uint8 and qb.scale.shape == qb.zero_point.shape == (6, 5, 1)
    one = optim.QuantizedBuffer.zeros((6, 32), "cpu")
    assert one.weight.shape == (6, 32) and one.scale.shape == (6, 1)
    meta, t = U.load("q8_f32_zero_group")  # the reference's tensors in the holder give the reference's dequantized values
    qb = optim.QuantizedBuffer(t["exp_avg_q3"], t["exp_avg_scale3"], t["exp_avg_zp3"], meta["shape"])
    assert torch.equal(qb.dequantize(), t["exp_avg_deq3"])
    assert qb.dequantize(torch.bfloat16).dtype == torch.bfloat16


def test_state_dict_round_trip(tmp_path):
    g = torch.Generator().manual_seed(3)
    dense, quant = _param((5, 7), torch.bfloat16), _param((8, 64))
    opt = optim.AdamW([dict(params=[dense], lr=0.5), dict(params=[quant], use_quantized_buffers=True, quantized_buffers_minimum_numel=256)])
    qb = [optim.QuantizedBuffer(torch.randint(0, 256, (8, 2, 32), generator=g).to(torch.uint8), torch.rand(8, 2, 1, generator=g),
                                torch.randn(8, 2, 1, generator=g), (8, 64)) for _ in range(2)]
    opt.state[dense] = dict(step=3, exp_avg=torch.randn(5, 7, generator=g).bfloat16(), exp_avg_sq=torch.rand(5, 7, generator=g).bfloat16())
    opt.state[quant] = dict(step=7, exp_avg=qb[0], exp_avg_sq=qb[1])
    path = tmp_path / "opt.pt"
    torch.save(opt.state_dict(), path)
    loaded = torch.load(path, weights_only=True)
    d2, q2 = _param((5, 7), torch.bfloat16), _param((8, 64))
    new = optim.AdamW([dict(params=[d2]), dict(params=[q2])])
    new.load_state_dict(loaded)
    assert new.param_groups[0]["lr"] == 0.5 and new.param_groups[1]["use_quantized_buffers"] is True
    assert new.state[d2]["step"] == 3 and new.state[q2]["step"] == 7
    for key in ("exp_avg", "exp_avg_sq"):
        assert new.state[d2][key].dtype == torch.bfloat16 and torch.equal(new.state[d2][key], opt.state[dense][key])
        a, b = new.state[q2][key], opt.state[quant][key]
        assert isinstance(a, optim.QuantizedBuffer) and a.shape == b.shape
        for x, y in zip(a.parts(), b.parts()):
            assert x.dtype == y.dtype and torch.equal(x, y) and x.data_ptr() != y.data_ptr()
    # a second generation gives the same dictionary
    again = new.state_dict()
    assert again["param_groups"] == opt.state_dict()["param_groups"]


def test_entry_points_validate_without_gpu():
    lib = _lib.load()
    buf = torch.zeros(64 + 16, dtype=torch.uint8)
    a = (buf.data_ptr() + 15) // 16 * 16
    tail = (1e-3, 0.1, 0.001, 0.1, 0.001, 1.0, 1.0, None, 0, 0, 0, 0, None)
    f, q = lib.sdnq_hip_adamw_step, lib.sdnq_hip_adamw_step_q8
    assert f(None, a, a, a, 0, 8, *tail) == -1                         # NULL
    assert f(a, a, a, a, 3, 8, *tail) == -2                            # dtype
    assert f(a, a, a, a, 0, 0, *tail) == -3                            # shape
    assert f(a + 4, a, a, a, 0, 8, *tail) == lib.sdnq_hip_colquant_t(a + 4, 0, 8, 8, 8, a, 16, a, None, a, 1 << 20, None)  # alignment
    assert q(a, a, 0, 48, a, a, a, a, a, a, *tail) == -3               # numel % 32
    assert q(a, a, 0, 64, None, a, a, a, a, a, *tail) == -1
    assert q(a, a, 0, 64, a + 8, a, a, a, a, a, *tail) == f(a + 4, a, a, a, 0, 8, *tail)
    nan_lr = (float("nan"),) + tail[1:]
    assert f(a, a, a, a, 0, 8, *nan_lr) != 0 and q(a, a, 0, 64, a, a, a, a, a, a, *nan_lr) != 0


@pytest.mark.parametrize("name", U.names())
def test_float64_restatement_reproduces_the_fixtures(name):
    """Bound (relative to the tensor's largest magnitude): the float32 chain of the reference, CHAIN_ROUNDINGS roundings of half an ulp,
    plus -- for 16-bit storage -- one ulp of the storage dtype, where the float32 and the float64 value fall on two sides of a rounding
    boundary.  Quantized state: every dequantized element within one quantization step (the group's scale) of the fixture's."""
    meta, t = U.load(name)
    assert meta["options"]["use_stochastic_rounding"] is False and meta["options"]["use_stochastic_buffers"] is False
    bound = U.F32_CHAIN + (U.REL_ULP[meta["dtype"]] if meta["dtype"] != "f32" else 0.0)
    for i in range(1, U.STEPS + 1):
        r = U.restate_fixture_step(name, i)
        d = U.distance(r["p"], t[f"p{i}"])
        print(name, "step", i, "p", d, "bound", bound)
        assert d <= bound
        for key in ("exp_avg", "exp_avg_sq"):
            if meta["quantized"]:
                assert U.deq_excess(r[key + "_deq"], t[f"{key}_deq{i}"], t[f"{key}_scale{i}"], meta["shape"]) == 0, (key, i)
                assert U.ulps_f32(r[key + "_scale"], t[f"{key}_scale{i}"]) <= 2 and U.ulps_f32(r[key + "_zp"], t[f"{key}_zp{i}"]) <= 2
            else:
                d = U.distance(r[key], t[f"{key}{i}"])
                print(name, "step", i, key, d)
                assert d <= bound
    if meta.get("zero_groups"):
        for row, grp in meta["zero_groups"]:
            assert t["exp_avg_scale3"][row, grp, 0] == 0 and int(t["exp_avg_q3"][row, grp].max()) == 0
