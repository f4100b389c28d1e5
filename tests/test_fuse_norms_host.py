"""fuse_norms / SDNQFusedNorm host logic and the status codes of sdnq_hip_norm_rowquant: no GPU needed."""
import ctypes

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, ops
from sdnq_amd.activations import FuseActivationsResult
from sdnq_amd.norms import FuseNormsResult, SDNQFusedNorm, fuse_norms, norm_kind, unfuse_norms


class LlamaRMSNorm(torch.nn.Module):
    def __init__(self, k, **attrs):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(k))
        for name, value in attrs.items():
            setattr(self, name, value)

    def forward(self, x):
        return self.weight * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)


def _model():
    return torch.nn.ModuleDict({
        "ln": torch.nn.LayerNorm(64), "rms": LlamaRMSNorm(32, variance_epsilon=1e-6), "odd": torch.nn.LayerNorm(20),
        "two_d": torch.nn.LayerNorm((4, 16)), "inner": torch.nn.Sequential(torch.nn.LayerNorm(16, elementwise_affine=False), torch.nn.Linear(16, 16))})


def test_default_targets_names_and_predicate():
    model = _model()
    assert sdnq_amd.fuse_norms is fuse_norms and sdnq_amd.unfuse_norms is unfuse_norms and sdnq_amd.SDNQFusedNorm is SDNQFusedNorm
    res = fuse_norms(model)
    assert res == 3 and res.fused == ["ln", "rms", "inner.0"] and all(isinstance(model[n], SDNQFusedNorm) for n in ("ln", "rms"))
    assert dict(res.skipped) == {"odd": "K = 20 is not a multiple of 8", "two_d": "normalizes over 2 trailing dimensions (one is built)"}
    assert fuse_norms(model) == 0 and unfuse_norms(model) == 3 and isinstance(model["ln"], torch.nn.LayerNorm)
    res = fuse_norms(model, targets=["rms", "inner.1", "nowhere"], mm="fp8")
    assert res.fused == ["rms"] and model["rms"].mm == ops.MM_FP8 and [n for n, _ in res.skipped] == ["inner.1", "nowhere"]
    assert "not a LayerNorm or an RMSNorm-shaped module" in res.skipped[0][1] and res.skipped[1][1] == "is not a submodule of the model"
    assert fuse_norms(model, targets=["rms"]).skipped == [("rms", "is fused already")]
    unfuse_norms(model)
    # a target inside an existing wrapper is the wrapper's: not wrapped a second time, and unfuse_norms restores the original object
    ln = model["ln"]
    assert fuse_norms(model) == 3
    res = fuse_norms(model, targets=["ln.norm"])
    assert res == 0 and res.fused == [] and res.skipped == [] and model["ln"].norm is ln and type(ln) is torch.nn.LayerNorm
    assert fuse_norms(model, targets=lambda name, mod: name == "ln").skipped == [("ln", "is fused already")]  # a predicate that matches a wrapper
    assert unfuse_norms(model) == 3 and model["ln"] is ln
    assert FuseNormsResult is FuseActivationsResult and isinstance(res, FuseNormsResult)
    assert fuse_norms(model, targets=lambda name, mod: name.startswith("inner")).fused == ["inner.0"]
    with pytest.raises(_lib.SdnqHipError):
        fuse_norms(model, mm="int4")


@pytest.mark.parametrize("mod, kind", [
    (LlamaRMSNorm(32, variance_epsilon=1e-6), (ops.NORM_RMS, 32)),
    (LlamaRMSNorm(32, eps=1e-5), (ops.NORM_RMS, 32)),
    (LlamaRMSNorm(32), None),                               # no epsilon
    (LlamaRMSNorm(32, eps=1e-5, bias=torch.zeros(32)), None),  # a bias
    (torch.nn.Linear(32, 32), None)])
def test_rmsnorm_shape_recognition(mod, kind):
    assert norm_kind(mod) == kind if kind else isinstance(norm_kind(mod), str)


def test_cpu_tensors_take_the_wrapped_forward():
    from sdnq_amd import linear as L
    ln = torch.nn.LayerNorm(64)
    fused, x = SDNQFusedNorm(ln), torch.randn(2, 5, 64)
    scale, shift = torch.randn(2, 64), torch.randn(2, 1, 64)
    with torch.no_grad():
        assert torch.equal(fused(x), ln(x))
        assert torch.equal(fused(x, scale, shift), ln(x) * (1 + scale[:, None]) + shift)
    assert not L._ts.act_cache.entries and L._ts.seed is None
    with pytest.raises(ValueError):
        fused(x, scale)


def test_status_codes_without_gpu():
    """Validation runs before any launch."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def call(x=p, x_dtype=1, k=64, ldx=64, norm=0, weight=None, bias=None, affine_dtype=0, scale=None, shift=None, rpb=0, ld_mod=0, mm=0, y=None, xq=p, xs=p):
        return lib.sdnq_hip_norm_rowquant(x, x_dtype, 4, k, ldx, norm, 1e-5, weight, bias, affine_dtype, scale, shift, rpb, ld_mod, mm, y, xq, xs, None)

    assert call(x=None) == _lib.ERR_NULL and call(xq=None) == _lib.ERR_NULL and call(bias=p) == _lib.ERR_NULL and call(scale=p) == _lib.ERR_NULL
    assert call(x_dtype=0) == _lib.ERR_DTYPE and call(mm=5) == _lib.ERR_DTYPE and call(weight=p, affine_dtype=2) == _lib.ERR_DTYPE
    assert call(k=60, ldx=60) == _lib.ERR_SHAPE and call(ldx=56) == _lib.ERR_SHAPE
    assert call(scale=p, shift=p, rpb=3, ld_mod=64) == _lib.ERR_SHAPE and call(scale=p, shift=p, rpb=2, ld_mod=56) == _lib.ERR_SHAPE
    assert call(x=p + 2) == _lib.ERR_ALIGN and call(ldx=68) == _lib.ERR_ALIGN and call(weight=p + 4) == _lib.ERR_ALIGN and call(y=p + 8) == _lib.ERR_ALIGN
    assert call(scale=p, shift=p, rpb=2, ld_mod=68) == _lib.ERR_ALIGN
    assert call(norm=2) == _lib.ERR_UNSUPPORTED and call(norm=1, weight=p, bias=p) == _lib.ERR_UNSUPPORTED
