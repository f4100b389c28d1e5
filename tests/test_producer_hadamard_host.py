"""Host logic of the rotated producers and the status codes of sdnq_hip_norm_rowquant_had / sdnq_hip_act_rowquant_had: no GPU needed."""
import ctypes

import pytest
import torch

from sdnq_amd import _lib, ops
from sdnq_amd.activations import fuse_activations
from sdnq_amd.norms import SDNQFusedNorm, fuse_norms


@pytest.fixture
def aligned():
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    yield p + (-p) % 16
    del buf


def test_status_codes_without_gpu(aligned):
    """Validation runs before any launch: the sibling's statuses, then the row quantizer's group rule."""
    lib, p = _lib.load(), aligned

    def norm(x=p, k=256, group=64, xq=p):
        return lib.sdnq_hip_norm_rowquant_had(x, 1, 4, k, k, 0, 1e-5, None, None, 0, None, None, 0, 0, 0, group, None, xq, p, None)

    def act(a=p, n=256, group=64, xq=p):
        return lib.sdnq_hip_act_rowquant_had(a, None, 1, 4, n, n, 0, 1, 0, group, None, xq, p, None)

    for call in (norm, act):
        assert call(None) == _lib.ERR_NULL and call(xq=None) == _lib.ERR_NULL
        assert call(group=48) == _lib.ERR_SHAPE and call(group=1024) == _lib.ERR_SHAPE and call(group=512) == _lib.ERR_SHAPE  # 256 % 512
        assert call(p + 2) == _lib.ERR_ALIGN and call(xq=p + 8) == _lib.ERR_ALIGN


class _Stub:
    """Stands in for the loaded library: notes the entry point called and answers `status`."""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.status if name.endswith("_had") else 0
        return fn


@pytest.mark.parametrize("group, status, names", [
    (0, 0, ["sdnq_hip_norm_rowquant", "sdnq_hip_act_rowquant"]),
    (64, 0, ["sdnq_hip_norm_rowquant_had", "sdnq_hip_act_rowquant_had"]),
    (64, -5, ["sdnq_hip_norm_rowquant_had", "sdnq_hip_norm_rowquant", "sdnq_hip_act_rowquant_had", "sdnq_hip_act_rowquant"])])
def test_ops_choose_the_entry_point(monkeypatch, group, status, names):
    rec = _Stub(status)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(ops, "_require_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda t: 0)
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    outs = [ops.norm_rowquant(x, ops.NORM_RMS, 1e-5, None, None, None, None, ops.MM_I8, hadamard_group=group),
            ops.act_rowquant(x, None, ops.ACT_SILU, ops.MM_I8, hadamard_group=group)]
    assert [name for name, _ in rec.calls] == names
    for y, xq, xs in outs:  # "not built" (-5): y alone, the consumer quantizes for itself
        assert y is not None and (xq is None) == (xs is None) == (status == -5)
    if group == 0:  # the plain symbols get exactly the plain arguments
        assert [len(args) for _, args in rec.calls] == [19, 13]
    elif status == 0:
        assert [args[-5] for _, args in rec.calls] == [group, group]


def test_a_group_the_rows_cannot_take_is_skipped():
    model = torch.nn.ModuleDict({"ln": torch.nn.LayerNorm(512), "ln320": torch.nn.LayerNorm(320), "act": torch.nn.GELU(approximate="tanh")})
    res = fuse_norms(model, hadamard_group=192)
    assert res == 0 and [n for n, _ in res.skipped] == ["ln", "ln320"] and all("192" in why for _, why in res.skipped)
    assert fuse_activations(model, hadamard_group=192).skipped[0][0] == "act"
    res = fuse_norms(model, hadamard_group=256)  # 320 % 256
    assert res.fused == ["ln"] and model["ln"].had == 256 and [n for n, _ in res.skipped] == ["ln320"]
    assert fuse_norms(torch.nn.ModuleDict({"ln": torch.nn.LayerNorm(512)})) == 1  # the default changes nothing
    with pytest.raises(ValueError):
        SDNQFusedNorm(torch.nn.LayerNorm(320), hadamard_group=256)
