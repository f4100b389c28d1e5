"""The grouped one-launch w8a8 Linear (sdnq_hip_linear_w8a8_fused_grouped, csrc/gemm_aq_kernel.h with AQ_GROUPED 1): several int8 layers
that read one activation in ONE launch of the direct 32 x 256 tile -- column block t of the launch is block t % bpm of member t / bpm, and
only the tile's base pointers (slab copy, scales, bias, output matrix) come from the member.

Expected values never come from the launch under test.  Every member's output must have the bits of two other routes:
  (a) ops.rowquant + ops.scaled_mm_grouped (the route the group took before), and
  (b) that member's own ops.linear_w8a8_fused call on its own slab copy.
Equality of bits, no tolerance.  Weights, scales and biases are distinct random draws per member, so a tile that reads another member's
slab, scale or bias, or writes into another member's matrix, changes bits.

Shapes: K = 768 (six stages, the smallest K the route accepts), 896 (seven: one past a multiple of the three register stages), 1280 (all
ten); n_member = 256 and 512 (one and two column blocks per member: the member boundary on a block edge and inside a walk group); 2 and 3
members; M = 33, 64, 95, 160 (ragged last row block; 2, 3 and 5 row blocks); bf16 and f16; every member with a bias and none.  On these
sizes no CU holds two tiles; the SDXL q / k / v group (1024 x 3 x 1280 x 1280: 480 tiles, more than any part has CUs) does."""
import pytest
import torch

from sdnq_amd import _lib

pytestmark = pytest.mark.gpu

from sdnq_amd import linear, ops  # noqa: E402

KS = [768, 896, 1280]
NS = [256, 512]
GS = [2, 3]
MS = [33, 64, 95, 160]
DTYPES = [torch.bfloat16, torch.float16]
I8, FP8 = ops.MM_I8, ops.MM_FP8


def _bits(t):
    return t.view(torch.int16)


def _members(g, n, k, m, seed, dev):
    """x in float32 (cast per case) and g members (b, sb, bias in float32), every one its own draw."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=gen) * torch.exp(torch.randn(m, 1, generator=gen))
    mem = []
    for _ in range(g):
        b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=gen)
        sb = torch.rand(n, generator=gen) * 0.02 + 1e-4
        bias = torch.randn(n, generator=gen)
        mem.append((b.to(dev), sb.to(dev), bias.to(dev)))
    return x.to(dev), mem


def _supported(mm, dtype, m, n, g, k):
    code = ops.float_code(dtype)
    return _lib.load().sdnq_hip_linear_w8a8_fused_grouped_supported(mm, code, code, m, n, g, k)


def _check(x, mem, slabs, dtype, with_bias, what):
    m, k = x.shape
    n, g = mem[0][0].shape[0], len(mem)
    biases = [bias.to(dtype) if with_bias else None for (_, _, bias) in mem]
    assert _supported(I8, dtype, m, n, g, k) == 1, what
    got = ops.linear_w8a8_fused_grouped(I8, x, [(s, sb, bi) for s, (_, sb, _), bi in zip(slabs, mem, biases)], dtype)
    xq, xs, _, _ = ops.rowquant(x, I8)
    two = ops.scaled_mm_grouped(I8, xq, xs, ops.GemmGroup([(b, sb, bi) for (b, sb, _), bi in zip(mem, biases)]), dtype)
    own = [ops.linear_w8a8_fused(I8, x, b, sb, bi, dtype, s) for (b, sb, _), bi, s in zip(mem, biases, slabs)]
    torch.cuda.synchronize()
    assert len(got) == g
    for i in range(g):
        assert got[i].shape == (m, n) and got[i].is_contiguous()
        assert torch.equal(_bits(got[i]), _bits(two[i])), ("vs rowquant + scaled_mm_grouped", what, i, int((_bits(got[i]) != _bits(two[i])).sum()))
        assert torch.equal(_bits(got[i]), _bits(own[i])), ("vs the member's own launch", what, i, int((_bits(got[i]) != _bits(own[i])).sum()))


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_every_member_has_the_bits_of_both_other_routes(k, n, g, gpu_device):
    xf, mem = _members(g, n, k, max(MS), 1009 * g + 17 * n + k, gpu_device)
    slabs = [ops.aq_slab_pack(b) for (b, _, _) in mem]
    for dtype in DTYPES:
        for m in MS:
            x = xf[:m].to(dtype)
            for with_bias in (True, False):
                _check(x, mem, slabs, dtype, with_bias, (m, n, g, k, dtype, with_bias))


def test_two_tiles_per_cu_the_sdxl_qkv_group(gpu_device):
    """480 tiles in a single launch: more than the part has CUs, so pairs of tiles share a CU."""
    m, n, g, k = 1024, 1280, 3, 1280
    assert (m // 32) * g * (n // 256) > torch.cuda.get_device_properties(gpu_device).multi_processor_count
    xf, mem = _members(g, n, k, m, 480, gpu_device)
    slabs = [ops.aq_slab_pack(b) for (b, _, _) in mem]
    _check(xf.to(torch.bfloat16), mem, slabs, torch.bfloat16, True, "sdxl q/k/v")


def test_strided_activation_rows(gpu_device):
    m, n, g, k = 95, 256, 3, 1280
    xf, mem = _members(g, n, k, m, 5, gpu_device)
    slabs = [ops.aq_slab_pack(b) for (b, _, _) in mem]
    wide = torch.full((m, k + 136), 3.0e4, dtype=torch.bfloat16, device=gpu_device)  # (a read past K would raise the row's amax)
    wide[:, :k] = xf.to(torch.bfloat16)
    got = ops.linear_w8a8_fused_grouped(I8, wide[:, :k], [(s, sb, None) for s, (_, sb, _) in zip(slabs, mem)], torch.bfloat16)
    own = [ops.linear_w8a8_fused(I8, xf.to(torch.bfloat16), b, sb, None, torch.bfloat16, s) for (b, sb, _), s in zip(mem, slabs)]
    torch.cuda.synchronize()
    for y, r in zip(got, own):
        assert torch.equal(_bits(y), _bits(r))


@pytest.mark.parametrize("mm, n, k, why", [
    (I8, 320, 1280, "n_member is no multiple of the 256-column block"),
    (I8, 256, 2048, "K = 2048: the rows do not stay resident"),
    (I8, 256, 640, "K = 640 belongs to the tall single-layer forms"),
    (FP8, 256, 1280, "fp8"),
])
def test_unsupported_groups_keep_the_two_launch_route(mm, n, k, why, gpu_device):
    """supported() says no, the entry point launches nothing (SDNQ_ERR_UNSUPPORTED), and the route such a group keeps -- the row quantizer
    and the grouped GEMM -- gives every member the bits of its own two-launch call."""
    m, g, dtype = 95, 2, torch.bfloat16
    assert _supported(mm, dtype, m, n, g, k) == 0, why
    xf, mem = _members(g, n, k, m, n + k, gpu_device)
    x = xf.to(dtype)
    if mm == FP8:
        mem = [(b.to(torch.float32).to(torch.float8_e4m3fn), sb, bias) for (b, sb, bias) in mem]
    fake_slabs = [torch.zeros(max(ops.aq_slab_bytes(n, k), 16), dtype=torch.int8, device=gpu_device) for _ in mem]
    with pytest.raises(_lib.SdnqHipError):
        ops.linear_w8a8_fused_grouped(mm, x, [(s, sb, None) for s, (_, sb, _) in zip(fake_slabs, mem)], dtype)
    xq, xs, _, _ = ops.rowquant(x, mm)
    two = ops.scaled_mm_grouped(mm, xq, xs, ops.GemmGroup([(b, sb, bias.to(dtype)) for (b, sb, bias) in mem]), dtype)
    torch.cuda.synchronize()
    for y, (b, sb, bias) in zip(two, mem):
        ref, _, _ = ops.linear_w8a8(mm, x, b, sb, bias.to(dtype), dtype)
        assert torch.equal(_bits(y), _bits(ref)), why


def test_members_of_unequal_width_keep_the_two_launch_route(gpu_device):
    """ProjectionGroup._slabs (the host's question) answers None for a group whose members differ in width, whatever supported() would say
    about either width: the group runs the row quantizer and the grouped GEMM, and those still match."""
    m, k, dtype = 64, 1280, torch.bfloat16
    xf, a = _members(1, 256, k, m, 31, gpu_device)
    _, b = _members(1, 512, k, m, 32, gpu_device)
    mem = a + b
    assert _supported(I8, dtype, m, 256, 2, k) == 1 and _supported(I8, dtype, m, 512, 2, k) == 1
    group = linear.ProjectionGroup.__new__(linear.ProjectionGroup)
    group.mods, group.states, group.pf_tensors = [None, None], (), ()
    group.gemm = ops.GemmGroup([(w, sb, bias.to(dtype)) for (w, sb, bias) in mem])
    x = xf.to(dtype)
    assert group._slabs(I8, x) is None
    xq, xs, _, _ = ops.rowquant(x, I8)
    two = ops.scaled_mm_grouped(I8, xq, xs, group.gemm, dtype)
    torch.cuda.synchronize()
    for y, (w, sb, bias) in zip(two, mem):
        ref, _, _ = ops.linear_w8a8(I8, x, w, sb, bias.to(dtype), dtype)
        assert torch.equal(_bits(y), _bits(ref))


def test_linked_layers_take_the_route_and_the_switches_give_the_two_launches_back(gpu_device, monkeypatch):
    """ProjectionGroup on three linked int8 layers: the first member called runs ONE grouped one-launch call on the 16-bit activation -- no
    ops.rowquant, the members' slab copies built once and kept in their states -- and every member's output has the bits of the layer run
    alone; with the slab copies switched off the group runs the row quantizer and the grouped GEMM, same bits."""
    import sdnq_amd
    from sdnq_amd import loader
    torch.manual_seed(3)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)

    def make_linear(k, n):
        lin = torch.nn.Linear(k, n, bias=True, device=gpu_device, dtype=torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(n, k, device=gpu_device) * 0.02)
        return sdnq_amd.sdnq_quantize_layer(lin, cfg)[0]

    mods = [make_linear(768, 256) for _ in range(3)]
    x = torch.randn(2, 48, 768, device=gpu_device, dtype=torch.bfloat16)
    monkeypatch.setattr(linear, "LINK_PROJECTIONS", False)
    alone = [m(x).clone() for m in mods]
    monkeypatch.setattr(linear, "LINK_PROJECTIONS", True)
    assert loader.link_layers(mods)
    group = mods[0].__dict__["_sdnq_group"][0]
    calls = {"rowquant": 0, "grouped": 0}
    real_rq, real_g = ops.rowquant, ops.linear_w8a8_fused_grouped
    monkeypatch.setattr(ops, "rowquant", lambda *a, **k: (calls.__setitem__("rowquant", calls["rowquant"] + 1), real_rq(*a, **k))[1])
    monkeypatch.setattr(ops, "linear_w8a8_fused_grouped", lambda *a, **k: (calls.__setitem__("grouped", calls["grouped"] + 1), real_g(*a, **k))[1])
    for step in range(2):
        linear.invalidate()
        for m, ref in zip(mods, alone):
            y = m(x)
            assert y.shape == ref.shape and torch.equal(_bits(y), _bits(ref))
    torch.cuda.synchronize()
    assert calls == {"rowquant": 0, "grouped": 2}
    slabs = [st.mm_slab for st in group.states]
    assert all(s is not None and s.numel() == 256 * 768 for s in slabs)
    monkeypatch.setattr(linear, "FUSED_ROWQUANT_SLABCOPY", False)
    linear.invalidate()
    for m, ref in zip(mods, alone):
        assert torch.equal(_bits(m(x)), _bits(ref))
    torch.cuda.synchronize()
    assert calls["grouped"] == 2 and calls["rowquant"] == 1
