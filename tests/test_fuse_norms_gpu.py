"""fuse_norms on a two-block toy: LayerNorm -> three int8 w8a8 Linears on one input, RMSNorm -> two.  The fused norms park their codes;
the Linears must give the bits of the unseeded route and launch no row quantizer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, K = 64, 256


class RMSNorm(torch.nn.Module):  # the shape of diffusers' / transformers' classes
    def __init__(self, k, eps=1e-6):
        super().__init__()
        self.weight = torch.nn.Parameter(1 + 0.1 * torch.randn(k))
        self.variance_epsilon = eps

    def forward(self, x):
        v = x.float().pow(2).mean(-1, keepdim=True)
        return (self.weight * (x.float() * torch.rsqrt(v + self.variance_epsilon))).to(x.dtype)


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        import sdnq_amd
        cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
        self.norm1, self.norm2 = torch.nn.LayerNorm(K).to(torch.bfloat16), RMSNorm(K).to(torch.bfloat16)
        for name in ("q", "k", "v", "gate", "up"):
            setattr(self, name, sdnq_amd.sdnq_quantize_layer(torch.nn.Linear(K, K).to(torch.bfloat16), cfg)[0])

    def forward(self, x):
        h = self.norm1(x)
        q, k, v = self.q(h), self.k(h), self.v(h)
        g = self.norm2(q)
        return torch.stack([q, k, v, self.gate(g), self.up(g)])


@pytest.fixture()
def toy():
    from sdnq_amd import linear as L
    torch.manual_seed(5)
    model = Toy().to("cuda:0").eval()
    x = (torch.randn(M, K) * 2 + 0.5).to(torch.bfloat16).to("cuda:0")
    L.clear_activation_cache()
    yield model, x
    L.clear_activation_cache()


def _bits(t):
    return t.contiguous().view(torch.int16)


def test_seeded_consumers_match_the_unseeded_route_and_launch_no_quantizer(toy):
    from sdnq_amd import linear as L
    from sdnq_amd.norms import SDNQFusedNorm, fuse_norms
    model, x = toy
    with torch.no_grad():
        assert fuse_norms(model).fused == ["norm1", "norm2"] and isinstance(model.norm1, SDNQFusedNorm)
        for norm, inp, layers in ((model.norm1, x, (model.q, model.k, model.v)), (model.norm2, x * 0.5, (model.gate, model.up))):
            h = norm(inp)
            entry = L._ts.act_cache.entries[-1]
            assert entry[0] is h and entry[5] is norm and not entry[6][0]
            seeded = [layer(h) for layer in layers]
            assert entry[6][0] and L._ts.act_cache.entries[-1] is entry and len(L._ts.act_cache.entries) == 1  # hits; nobody quantized and parked
            L.clear_activation_cache()
            for layer, out in zip(layers, seeded):  # the unseeded route on the same y
                assert torch.equal(_bits(layer(h)), _bits(out))
            L.clear_activation_cache()


def test_one_launch_consumer_gives_the_same_bits_seeded(toy):
    from sdnq_amd import linear as L
    from sdnq_amd import ops
    from sdnq_amd.norms import fuse_norms
    model, x = toy
    fused_calls = ops.fused_call_count  # (the Python forward's and the C++ plans')
    with torch.no_grad():
        fuse_norms(model, targets=["norm1"])
        model.q.__dict__["_sdnq_unshared"] = L.UNSHARED_AFTER  # a layer whose parked codes nobody ever used: the one-launch route
        h = model.norm1(x).clone()
        L.clear_activation_cache()
        before = fused_calls()
        unseeded = [model.q(h), model.q(h)]  # the Python forward, then its C++ plan where that is built
        assert fused_calls() == before + 2
        h2 = model.norm1(x)
        entry = L._ts.act_cache.entries[-1]
        seeded = model.q(h2)
        assert fused_calls() == before + 2 and entry[6][0]
        assert torch.equal(_bits(h2), _bits(h)) and all(torch.equal(_bits(seeded), _bits(u)) for u in unseeded)


def test_unfuse_fallbacks_and_capture(toy):
    import sdnq_amd
    from sdnq_amd import linear as L
    from sdnq_amd.norms import fuse_norms, unfuse_norms
    model, x = toy
    norm1, norm2 = model.norm1, model.norm2
    with torch.no_grad():
        plain = model(x)
        L.clear_activation_cache()
        fuse_norms(model)
        fused = model(x)
        L.clear_activation_cache()
    # gradients required, inference-mode tensors: the wrapped norm's own output, nothing parked
    xg = x.clone().requires_grad_(True)
    assert torch.equal(_bits(model.norm1(xg).detach()), _bits(norm1(xg).detach())) and not L._ts.act_cache.entries
    with torch.inference_mode():
        assert torch.equal(_bits(model.norm1(x)), _bits(norm1(x))) and not L._ts.act_cache.entries
    # a captured step replays to the eager bits
    captured = sdnq_amd.capture(model, x)
    for _ in range(3):
        assert torch.equal(_bits(captured(x)), _bits(fused))
    # unfuse_norms: the original modules and their bits
    assert unfuse_norms(model) == 2 and model.norm1 is norm1 and model.norm2 is norm2
    with torch.no_grad():
        assert torch.equal(_bits(model(x)), _bits(plain))
