"""fuse_activations / SDNQFusedActivation host logic and the status codes of sdnq_hip_act_rowquant: no GPU needed."""
import ctypes

import pytest
import torch

import sdnq_amd
from sdnq_amd import _lib, ops
from sdnq_amd.activations import SDNQFusedActivation, fuse_activations, unfuse_activations


class GEGLU(torch.nn.Module):  # the shape of diffusers' class
    def __init__(self, k, n):
        super().__init__()
        self.proj = torch.nn.Linear(k, 2 * n)

    def forward(self, x):
        h, gate = self.proj(x).chunk(2, dim=-1)
        return h * torch.nn.functional.gelu(gate)


class ApproximateGELU(GEGLU):  # diffusers' x * sigmoid(1.702 x) by name: not built, never run here
    pass


class MLP(torch.nn.Module):
    def __init__(self, k, n, act_fn):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = torch.nn.Linear(k, n), torch.nn.Linear(k, n), torch.nn.Linear(n, k), act_fn

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


def _model():
    return torch.nn.ModuleDict({
        "ff": torch.nn.Sequential(GEGLU(16, 32), torch.nn.Dropout(0.0), torch.nn.Linear(32, 16)), "mlp": MLP(16, 24, torch.nn.SiLU()),
        "act": torch.nn.GELU(approximate="tanh"), "quick": ApproximateGELU(16, 16), "odd": GEGLU(16, 12), "relu_mlp": MLP(16, 24, torch.nn.ReLU())})


def test_targets_kinds_and_unfuse():
    model = _model()
    originals = {n: model[n] for n in ("mlp", "act")}
    assert (sdnq_amd.fuse_activations, sdnq_amd.unfuse_activations, sdnq_amd.SDNQFusedActivation) == (fuse_activations, unfuse_activations, SDNQFusedActivation)
    res = fuse_activations(model)
    assert res == 3 and res.fused == ["ff.0", "mlp", "act"] and isinstance(model["ff"][0], SDNQFusedActivation)  # mlp.act_fn is the wrapper's
    assert [(m.shape, m.act, m.gated) for m in (model["ff"][0], model["mlp"], model["act"])] == [
        ("proj", ops.ACT_GELU, True), ("mlp", ops.ACT_SILU, True), ("plain", ops.ACT_GELU_TANH, False)]
    skipped = dict(res.skipped)
    assert set(skipped) == {"quick", "odd", "relu_mlp"} and skipped["odd"] == "N = 24 / 2 is not a multiple of 8"
    assert "is not a GELU / SiLU" in skipped["quick"] and skipped["relu_mlp"].startswith("its act_fn is a ReLU")
    assert fuse_activations(model) == 0 and fuse_activations(model, targets=["act"]).skipped == [("act", "is fused already")]
    res = fuse_activations(model, targets=["mlp.module.act_fn"])  # inside an existing wrapper: the wrapper's
    assert res == 0 and res.fused == [] and res.skipped == [] and type(model["mlp"].module.act_fn) is torch.nn.SiLU
    assert fuse_activations(model, targets=lambda name, mod: name == "act").skipped == [("act", "is fused already")]
    assert unfuse_activations(model) == 3 and all(model[n] is m for n, m in originals.items()) and isinstance(model["ff"][0], GEGLU)
    res = fuse_activations(model, targets=["mlp.act_fn", "ff.2", "nowhere"], mm="fp8")
    assert res.fused == ["mlp.act_fn"] and model["mlp"].act_fn.mm == ops.MM_FP8 and [n for n, _ in res.skipped] == ["ff.2", "nowhere"]
    unfuse_activations(model)
    assert fuse_activations(model, targets=lambda name, mod: name == "ff.0").fused == ["ff.0"]
    with pytest.raises(_lib.SdnqHipError):
        fuse_activations(model, mm="int4")


def test_cpu_tensors_take_the_wrapped_forward():
    from sdnq_amd import linear as L
    torch.manual_seed(0)
    model = _model()
    x = torch.randn(2, 5, 16)
    L.clear_activation_cache()  # (whatever earlier tests parked)
    with torch.no_grad():
        plain = [model["ff"](x), model["mlp"](x), model["act"](x)]
        fuse_activations(model)
        assert all(torch.equal(a, b) for a, b in zip([model["ff"](x), model["mlp"](x), model["act"](x)], plain))
    assert not L._ts.act_cache.entries and L._ts.seed is None


def test_status_codes_without_gpu():
    """Validation runs before any launch."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def call(a=p, b=None, x_dtype=1, n=64, lda=64, ldb=0, act=0, mm=0, y=None, xq=p, xs=p):
        return lib.sdnq_hip_act_rowquant(a, b, x_dtype, 4, n, lda, ldb, act, mm, y, xq, xs, None)

    assert call(a=None) == _lib.ERR_NULL and call(xq=None) == _lib.ERR_NULL and call(xs=None, y=p) == _lib.ERR_NULL
    assert call(x_dtype=0) == _lib.ERR_DTYPE and call(mm=5) == _lib.ERR_DTYPE
    assert call(n=60, lda=60) == _lib.ERR_SHAPE and call(lda=56) == _lib.ERR_SHAPE and call(b=p, ldb=56) == _lib.ERR_SHAPE
    assert call(a=p + 2) == _lib.ERR_ALIGN and call(lda=68) == _lib.ERR_ALIGN and call(b=p, ldb=68) == _lib.ERR_ALIGN and call(y=p + 8) == _lib.ERR_ALIGN
    assert call(act=3) == _lib.ERR_UNSUPPORTED
