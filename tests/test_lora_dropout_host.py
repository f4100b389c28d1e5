"""LoRA dropout on the Linear adapters, host side: the three new exports and their argument checks against their plain siblings', the
checks of the ops wrappers, add_lora(dropout=...) / remove_lora on a model built on the CPU, the threshold and scale arithmetic, and the
mask the oracle predicts for a fixed (seed, offset)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import sdnq_amd
from oracle import oracle as O
from sdnq_amd import _lib, lora, ops
from tests import lora_util as L
from tests.test_lora_host import QUANTIZED, toy_model

NEW = {"sdnq_hip_lowrank_down_dropout": 12, "sdnq_hip_lowrank_add_dropout": 13, "sdnq_hip_lowrank_grad_dropout": 17}
STREAM = 5   # the Philox stream of the dropout mask (the AdamW step uses 0 .. 4)


def test_the_three_symbols_are_declared_exported_and_bound():
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    for name, arity in NEW.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(raw, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name
        assert fn.argtypes[-4] is ctypes.c_int and fn.argtypes[-3] is ctypes.c_uint64 and fn.argtypes[-2] is ctypes.c_uint64, name
    assert callable(ops.lowrank_down_dropout) and callable(ops.lowrank_add_dropout) and callable(ops.lowrank_grad_dropout)


def test_statuses_are_the_plain_siblings():
    """Validation runs before any launch: every broken argument gets the status the plain entry point returns for it."""
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    drop = dict(thr=6554, seed=1, off=(1 << 32) + 4)
    # ---- add
    ok = dict(t=p, up=p, dt=_lib.BF16, rank=16, scale=1.0, y=p, m=5, n=16, ldy=16)
    cases = (dict(t=None), dict(up=None), dict(y=None), dict(dt=_lib.F32), dict(dt=7), dict(rank=12), dict(rank=0), dict(rank=264),
             dict(n=12, ldy=12), dict(ldy=8), dict(m=0), dict(t=p + 8), dict(up=p + 2), dict(y=p + 8), dict(ldy=20))
    for broken in cases:
        plain = raw.sdnq_hip_lowrank_add(*{**ok, **broken}.values(), None)
        got = raw.sdnq_hip_lowrank_add_dropout(*{**ok, **broken}.values(), *drop.values(), None)
        assert plain < 0 and got == plain, (broken, plain, got)
    for thr in (0, 65536, -1):
        assert raw.sdnq_hip_lowrank_add_dropout(*ok.values(), thr, 1, 4, None) == -3, thr
    # ---- grad
    okg = dict(a=p, lda=16, b=p, dt=_lib.F16, m=5, p=16, rank=8, scale=1.0, out_t=0, out=p, odt=_lib.F32, ws=None, wsb=0)
    many = L.LRG_SLAB + 1
    cases = (dict(a=None), dict(b=None), dict(out=None), dict(dt=_lib.F32), dict(odt=3), dict(odt=-1), dict(p=12, lda=12), dict(lda=8),
             dict(rank=12), dict(rank=512), dict(m=0), dict(out_t=2), dict(a=p + 8), dict(b=p + 4), dict(lda=20), dict(out=p + 2),
             dict(m=many), dict(m=many, ws=p, wsb=2 * 16 * 8 * 4 - 1), dict(m=many, ws=p + 4, wsb=1 << 12))
    for broken in cases:
        plain = raw.sdnq_hip_lowrank_grad(*{**okg, **broken}.values(), None)
        got = raw.sdnq_hip_lowrank_grad_dropout(*{**okg, **broken}.values(), *drop.values(), None)
        assert plain < 0 and got == plain, (broken, plain, got)
    for thr in (0, 65536, -1):
        assert raw.sdnq_hip_lowrank_grad_dropout(*okg.values(), thr, 1, 4, None) == -3, thr
    # ---- down: the matrix-core path of sdnq_hip_lowrank_down only -- what sends the plain call to its float32 / few-row fallback is
    # a dtype / shape status here
    okd = dict(x=p, dt=_lib.BF16, m=5, k=32, ldx=32, down=p, rank=16, t=p)
    down = raw.sdnq_hip_lowrank_down_dropout

    def rd(**broken):
        return down(*{**okd, **broken}.values(), *drop.values(), None)

    def plain_down(**broken):
        a = {**okd, **broken}
        return raw.sdnq_hip_lowrank_down(a["x"], a["dt"], a["m"], a["k"], a["ldx"], a["down"], a["dt"], a["rank"], a["t"], None)
    # (null, rank and alignment errors: the plain call validates these -- on the way to its fallback; it does not validate m or ldx)
    for broken in (dict(x=None), dict(down=None), dict(t=None), dict(rank=0), dict(x=p + 8), dict(down=p + 8), dict(ldx=36)):
        assert plain_down(**broken) < 0 and rd(**broken) == plain_down(**broken), broken
    assert rd(x=None) == -1 and rd(rank=0) == -3 and rd(x=p + 8) == -4 and rd(ldx=16) == -3 and rd(rank=-8) == -3
    assert rd(dt=_lib.F32) == -2 and rd(dt=7) == -2                 # no float32 path; an unknown dtype code
    assert rd(k=24, ldx=24) == -3 and rd(k=8, ldx=8) == -3           # 16 | K: no few-row fallback
    assert rd(m=0) == -3 and rd(m=-5) == -3
    assert rd(thr=0) == -3 and rd(thr=65536) == -3 and rd(thr=-1) == -3


def test_ops_checks_name_what_is_wrong():
    bf = torch.bfloat16
    t, up, y = torch.zeros(5, 16, dtype=bf), torch.zeros(24, 16, dtype=bf), torch.zeros(5, 24, dtype=bf)
    x, down = torch.zeros(5, 32, dtype=bf), torch.zeros(16, 32, dtype=bf)
    err = _lib.SdnqHipError
    d = (6554, 1, 4)
    with pytest.raises(err, match="CPU"):
        ops.lowrank_add_dropout(t, up, y, 1.0, *d)
    with pytest.raises(err, match="CPU"):
        ops.lowrank_grad_dropout(y, t, 1.0, *d)
    with pytest.raises(err, match="CPU"):
        ops.lowrank_down_dropout(x, down, *d)
    with pytest.raises(err, match="lowrank_add_dropout.*float32"):
        ops.lowrank_add_dropout(t.float(), up.float(), y.float(), 1.0, *d)
    with pytest.raises(err, match="lowrank_grad_dropout.*float32"):
        ops.lowrank_grad_dropout(y.float(), t.float(), 1.0, *d)
    with pytest.raises(err, match="lowrank_down_dropout.*float32"):
        ops.lowrank_down_dropout(x.float(), down.float(), *d)
    with pytest.raises(err, match=r"up must have the dtype"):
        ops.lowrank_add_dropout(t, up.half(), y, 1.0, *d)
    with pytest.raises(err, match=r"down must have the dtype"):
        ops.lowrank_down_dropout(x, down.half(), *d)
    with pytest.raises(err, match=r"rank = 12"):
        ops.lowrank_add_dropout(t[:, :12].contiguous(), up[:, :12].contiguous(), y, 1.0, *d)
    with pytest.raises(err, match=r"rank = 12"):
        ops.lowrank_grad_dropout(y, t[:, :12].contiguous(), 1.0, *d)
    with pytest.raises(err, match=r"rank = 12"):
        ops.lowrank_down_dropout(x, down[:12], *d)
    with pytest.raises(err, match=r"n = 20"):
        ops.lowrank_add_dropout(t, up[:20], y[:, :20], 1.0, *d)
    with pytest.raises(err, match=r"p = 20"):
        ops.lowrank_grad_dropout(y[:, :20], t, 1.0, *d)
    with pytest.raises(err, match=r"k = 24"):
        ops.lowrank_down_dropout(torch.zeros(5, 24, dtype=bf), torch.zeros(16, 24, dtype=bf), *d)
    with pytest.raises(err, match="y is misaligned"):
        ops.lowrank_add_dropout(t, up[:16], torch.zeros(5, 32, dtype=bf)[:, 4:20], 1.0, *d)
    with pytest.raises(err, match="a is misaligned"):
        ops.lowrank_grad_dropout(torch.zeros(5, 28, dtype=bf)[:, :24], t, 1.0, *d)
    with pytest.raises(err, match="x is misaligned"):
        ops.lowrank_down_dropout(torch.zeros(5, 36, dtype=bf)[:, :32], down, *d)
    with pytest.raises(err, match="t and up must be contiguous"):
        ops.lowrank_add_dropout(torch.zeros(5, 32, dtype=bf)[:, :16], up, y, 1.0, *d)
    with pytest.raises(err, match="down must be contiguous"):
        ops.lowrank_down_dropout(x, torch.zeros(16, 64, dtype=bf)[:, :32], *d)
    with pytest.raises(err, match=r"y \[M, N\]"):
        ops.lowrank_add_dropout(t, up, y[:4], 1.0, *d)
    with pytest.raises(err, match="same rows"):
        ops.lowrank_grad_dropout(y, t[:4], 1.0, *d)
    with pytest.raises(err, match=r"x \[M, K\]"):
        ops.lowrank_down_dropout(x, down[:, :16].contiguous(), *d)
    for call in (lambda thr, s, o: ops.lowrank_add_dropout(t, up, y, 1.0, thr, s, o), lambda thr, s, o: ops.lowrank_grad_dropout(y, t, 1.0, thr, s, o),
                 lambda thr, s, o: ops.lowrank_down_dropout(x, down, thr, s, o)):
        with pytest.raises(err, match="threshold = 0"):
            call(0, 1, 4)
        with pytest.raises(err, match="threshold = 65536"):
            call(65536, 1, 4)
        with pytest.raises(err, match="unsigned 64-bit"):
            call(6554, -1, 4)
        with pytest.raises(err, match="unsigned 64-bit"):
            call(6554, 1, 1 << 64)


def test_add_lora_checks_keeps_and_removes_dropout():
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dropout"):
            sdnq_amd.add_lora(toy_model(), rank=8, dropout=bad)
    m = toy_model()
    before = {n: getattr(m, n).forward_func for n in QUANTIZED}
    params = {k for k, _ in m.named_parameters()}
    with pytest.raises(NotImplementedError, match="conv adapters"):
        sdnq_amd.add_lora(m, rank=8, convs=True, dropout=0.1)
    assert all(getattr(m, n).forward_func is before[n] for n in QUANTIZED)          # the check runs before any module is touched
    assert {k for k, _ in m.named_parameters()} == params
    assert not any(hasattr(getattr(m, n), a) for n in QUANTIZED for a in ("lora_down", "lora_dropout", "lora_scale"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert sdnq_amd.add_lora(m, rank=8, convs=True, dropout=0.0) == 3            # dropout = 0 with convs is served as before
        assert m.conv.lora_dropout == 0.0
        sdnq_amd.remove_lora(m)
        assert sdnq_amd.add_lora(m, rank=8, alpha=16, dropout=0.25) == 2
    assert m.q.lora_dropout == 0.25 and m.k.lora_dropout == 0.25 and m.q.lora_scale == 2.0
    assert not hasattr(m.odd, "lora_dropout")
    twin = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(twin, rank=8)
    assert twin.q.lora_dropout == 0.0                                               # the default
    assert sdnq_amd.remove_lora(m) == 2
    assert not any(hasattr(m.q, a) for a in ("lora_down", "lora_up", "lora_scale", "lora_dropout"))


def test_cpu_forward_raises_in_training_mode_too():
    m = toy_model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sdnq_amd.add_lora(m, rank=8, dropout=0.5)
    x = torch.randn(40, 64, dtype=torch.bfloat16)
    m.train()
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        m.q(x)
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        with torch.no_grad():
            m.q(x)


def test_threshold_and_scale_arithmetic():
    """T = min(65535, max(1, round(p 65536))); scale_d = float32(scale 65536 / (65536 - T)) with the quotient in double."""
    want = {0.1: 6554, 0.5: 32768, 1e-6: 1, 0.99999: 65535}
    for p, t in want.items():
        assert lora.dropout_threshold(p) == t, p
        for scale in (1.0, 2.0, 1.5, 0.3):
            sd = lora.dropout_scale(scale, t)
            assert sd == float(np.float32(np.float64(scale) * 65536.0 / np.float64(65536 - t))), (p, scale)
            assert np.float32(sd) == sd                                             # a float32 value: the kernels get exactly this
    assert lora.dropout_scale(2.0, 32768) == 4.0 and lora.dropout_scale(1.0, 65535) == 65536.0
    assert lora.dropout_scale(1.0, 1) == float(np.float32(65536.0 / 65535.0))
    assert abs(want[0.1] / 65536 - 0.1) <= 2.0 ** -17                               # the effective probability


def test_the_predicted_mask_of_a_fixed_seed_and_offset():
    """The mask is oracle.adamw_halves(numel, seed, offset, 5) >= T.  The counts below were worked out once with the oracle's Philox
    (which tests/test_optim_oracle.py holds to the published test vectors): 40 x 136 elements, seed 1234, offset 2^32 + 8."""
    numel, seed, offset = 40 * 136, 1234, (1 << 32) + 8
    h = O.adamw_halves(numel, seed, offset, STREAM)
    assert h.shape == (numel,) and h.dtype == np.uint32 and int(h.max()) < 65536
    assert [int(v) for v in h[:8]] == [39752, 44028, 37257, 11188, 50512, 22982, 11782, 34889]
    assert int((h >= 6554).sum()) == 4919 and int((h >= 32768).sum()) == 2663
    assert int((O.adamw_halves(numel, seed, offset + 1, STREAM) >= 6554).sum()) == 4866   # the next offset: another mask
    assert int((O.adamw_halves(numel, seed, offset, 0) >= 6554).sum()) == 4897             # stream 0 (the AdamW parameter store): another
    # element e takes half e & 1 of word (e % 8) >> 1 of the call for e / 8
    w = O.adamw_words(numel, seed, offset, STREAM)
    e = 8 * 77 + 5
    assert int(h[e]) == int(w[77, 2] >> 16) and int(h[e - 1]) == int(w[77, 2] & 0xFFFF)
