"""The fused AdamW step on the MI355X (sdnq_amd.optim, csrc/optim.hip) against the reference's fixtures (tests/golden/optim_adamw_*) and
the float64 restatement of tests/optim_util.py.  The bounds are worked out in the tests' docstrings; the measured distances are printed
before they are asserted (profiles/optim_adamw_accuracy.md has both sides of them).  These tests check what the step and its stochastic
rounding are FOR (distances, unbiasedness); which bits they produce -- state bit-equal to the float32 oracle, the parameter within the
interval the 1-ulp rsqrt leaves, stochastic stores predicted from (seed, offset, element, stream) -- is tests/test_optim_exact_gpu.py."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFF = dict(use_stochastic_rounding=False, use_stochastic_buffers=False)
DENSE = [n for n in U.names() if not U.load(n)[0]["quantized"]]
QUANT = [n for n in U.names() if U.load(n)[0]["quantized"]]


def _optim():
    from sdnq_amd import optim
    return optim


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.uint8))


def fixture_optimizer(name, i):
    """(optimizer, parameter) holding the fixture's parameter, gradient and state in front of step i, made through the public interface."""
    O = _optim()
    meta, t = U.load(name)
    p = torch.nn.Parameter(t[f"p{i - 1}"].clone().to(DEV))
    p.grad = t[f"g{i}"].clone().to(DEV)
    opts = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["options"].items()}
    opt = O.AdamW([p], **opts)
    assert opts["use_stochastic_rounding"] is False and opts["use_stochastic_buffers"] is False
    if meta["grad_scale"] is not None:
        opt.grad_scale = torch.tensor(meta["grad_scale"], dtype=torch.float32, device=DEV)
    if i > 1:
        s = U.state_before(meta, t, i)
        if meta["quantized"]:
            opt.state[p] = dict(step=i - 1, **{k: O.QuantizedBuffer(s[k + "_q"].clone().to(DEV), s[k + "_scale"].clone().to(DEV),
                                                                  s[k + "_zp"].clone().to(DEV), meta["shape"]) for k in ("exp_avg", "exp_avg_sq")})
        else:
            opt.state[p] = dict(step=i - 1, exp_avg=s["exp_avg"].clone().to(DEV), exp_avg_sq=s["exp_avg_sq"].clone().to(DEV))
    return opt, p


def float_bound(name, key, i, ref_d):
    """Twice the reference's own distance from the restatement, plus one ulp of the storage dtype at the tensor's magnitude scale."""
    return 2.0 * ref_d[(key, i)] + U.REL_ULP[U.load(name)[0]["dtype"]]


@pytest.mark.parametrize("name", DENSE)
def test_deterministic_step_dense_state(name):
    """Each of the fixture's three steps, started from the fixture's state in front of it.  Bound per tensor, as max |err| / max |ref|
    against the float64 restatement: twice the distance of the reference's stored result from the same restatement (the operations are
    the same, contraction may differ) plus one ulp of the storage dtype."""
    meta, t = U.load(name)
    ref_d = U.reference_distances(name)
    for i in range(1, U.STEPS + 1):
        opt, p = fixture_optimizer(name, i)
        opt.step()
        st = opt.state[p]
        assert st["step"] == i and st["exp_avg"].dtype == p.dtype and st["exp_avg"].shape == p.shape
        r = U.restate_fixture_step(name, i)
        for key, got in (("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
            got = got.cpu()
            assert bool(torch.isfinite(got.float()).all())
            d, bound = U.distance(got, r[key]), float_bound(name, key, i, ref_d)
            same = (bits(got) == bits(t[f"{key}{i}"])).double().mean().item()
            print(f"accuracy {name} step {i} {key}: gpu {d:.3g} reference {ref_d[(key, i)]:.3g} bound {bound:.3g} bit-equal to fixture {same:.4f}")
            assert d <= bound, (name, i, key, d, bound)


@pytest.mark.parametrize("name", QUANT)
def test_deterministic_step_quantized_state(name):
    """As above for the parameter.  State: every dequantized element within one quantization step (the fixture's scale of its group) of
    the fixture's dequantized value, scales and zero points within 2 float32 ulp, and the share of codes that differ from the fixture at
    most twice the same share of the float64 restatement, with a floor of 0.1 %."""
    meta, t = U.load(name)
    ref_d = U.reference_distances(name)
    for i in range(1, U.STEPS + 1):
        opt, p = fixture_optimizer(name, i)
        opt.step()
        st = opt.state[p]
        r = U.restate_fixture_step(name, i)
        d, bound = U.distance(p.detach().cpu(), r["p"]), float_bound(name, "p", i, ref_d)
        print(f"accuracy {name} step {i} p: gpu {d:.3g} reference {ref_d[('p', i)]:.3g} bound {bound:.3g}")
        assert d <= bound
        for key in ("exp_avg", "exp_avg_sq"):
            qb = st[key]
            assert qb.weight.shape == t[f"{key}_q{i}"].shape and qb.scale.shape == t[f"{key}_scale{i}"].shape
            assert U.deq_excess(qb.dequantize().cpu(), t[f"{key}_deq{i}"], t[f"{key}_scale{i}"], meta["shape"]) == 0
            us, uz = U.ulps_f32(qb.scale.cpu(), t[f"{key}_scale{i}"]), U.ulps_f32(qb.zero_point.cpu(), t[f"{key}_zp{i}"])
            share = (qb.weight.cpu() != t[f"{key}_q{i}"]).double().mean().item()
            cap = max(2.0 * ref_d[("code_share", key, i)], 1e-3)
            print(f"accuracy {name} step {i} {key}: scale ulp {us} zero-point ulp {uz} code share {share:.3g} "
                  f"restatement {ref_d[('code_share', key, i)]:.3g} cap {cap:.3g}")
            assert us <= 2 and uz <= 2 and share <= cap
    if meta.get("zero_groups"):
        for row, grp in meta["zero_groups"]:
            assert float(st["exp_avg"].scale[row, grp, 0]) == 0 and int(st["exp_avg"].weight[row, grp].max()) == 0


def test_stochastic_rounding_of_a_bf16_parameter_and_state():
    """One step of a bf16 [256, 256] parameter from zero state.  The float32 values that get rounded are known exactly: the float32
    kernel computes the same chain from the same (bf16, hence float32-exact) inputs and stores it unrounded.  With beta1 = 0.5 - 2^-10
    and positive gradients exp_avg = (0.5 + 2^-10) g sits between a quarter and half a bf16 ulp ABOVE a grid point in every element:
    the source on which round-to-nearest is biased.  Checks, for parameter, exp_avg and exp_avg_sq: every stored value is one of the
    two bf16 neighbours of the float32 value; the mean of (stored - exact) is within 4 sigma / sqrt(n) of zero, sigma from the exact
    per-element residues (stored - exact is a two-point variable: up with probability residue / ulp); the same (seed, offset) repeats
    the bits; another offset gives others.  Round-to-nearest fails the mean check on exp_avg."""
    from sdnq_amd import ops
    n, ulp_bits = 256 * 256, 1 << 16
    g = torch.Generator().manual_seed(6)
    p0 = (torch.randn(256, 256, generator=g) * 0.5).bfloat16()
    gr = (torch.randn(256, 256, generator=g).abs() * 0.3 + 0.01).bfloat16()
    kw = dict(step=1, lr=2.0 ** -5, weight_decay=2.0 ** -5, betas=(0.5 - 2.0 ** -10, 0.999))
    pf, mf, vf = p0.float().to(DEV), torch.zeros(256, 256, device=DEV), torch.zeros(256, 256, device=DEV)
    ops.adamw_step(pf, gr.float().to(DEV), mf, vf, **kw)
    exact = dict(p=pf.cpu(), m=mf.cpu(), v=vf.cpu())

    def step(seed, offset, sr):
        p = p0.clone().to(DEV)
        m, v = (torch.zeros(256, 256, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        ops.adamw_step(p, gr.to(DEV), m, v, sr_param=sr, sr_state=sr, seed=seed, offset=offset, **kw)
        return dict(p=p.cpu(), m=m.cpu(), v=v.cpu())

    a, again, other, rne = step(1234, 8, True), step(1234, 8, True), step(1234, 12, True), step(1234, 8, False)
    for key in ("p", "m", "v"):
        x = exact[key].view(-1)
        lo = (x.view(torch.int32) & -ulp_bits).view(torch.float32)                # the neighbour towards zero
        hi = ((x.view(torch.int32) & -ulp_bits) + ulp_bits).view(torch.float32)   # the neighbour away from zero
        frac = (x.double() - lo.double()) / (hi.double() - lo.double())           # P(stored == hi) under the bit trick
        sigma = ((hi.double() - lo.double()) ** 2 * frac * (1 - frac)).sum().sqrt().item() / n
        got, near = a[key].float().view(-1), rne[key].float().view(-1)
        assert bool(((got == lo) | (got == hi)).all()) and bool(((near == lo) | (near == hi)).all()), key
        mean, mean_rne = (got.double() - x.double()).mean().item(), (near.double() - x.double()).mean().item()
        print(f"stochastic {key}: off-grid share {(frac > 0).double().mean().item():.3f} mean error {mean:.3g}, "
              f"4 sigma / sqrt(n) {4 * sigma:.3g}, round-to-nearest mean error {mean_rne:.3g}")
        assert (frac > 0).double().mean().item() > 0.9, key
        assert abs(mean) <= 4 * sigma, key
        assert torch.equal(bits(a[key]), bits(again[key])), key
        assert not torch.equal(bits(a[key]), bits(other[key])), key
        if key == "m":
            assert bool(((frac >= 0.25) & (frac < 0.5)).all()) and abs(mean_rne) > 4 * sigma


def test_stochastic_rounding_of_a_uint8_buffer():
    """quantize_weight(use_stochastic_rounding=True) restated: code = clamp(round(q + 0.1 z), 0, 255) with z standard normal, q = (x -
    min) / scale.  The kernel's z comes from Box-Muller on 24-bit uniforms, |z| <= sqrt(48 ln 2) = 5.77, so |code - q| <= 0.5 + 0.577.
    The number of codes that differ from round(q) is a sum of Bernoulli variables with p = P(round(q + 0.1 z) != round(q)), known per
    element: it lies within 4 sigma of its expectation (round-to-nearest gives 0 and fails), the mean of (code - q) within 4 sigma / sqrt(n)
    of its expectation; the same (seed, offset) repeats the codes, another offset gives others."""
    from sdnq_amd import ops
    O = _optim()
    shape = (256, 256)
    g = torch.Generator().manual_seed(9)
    gr = (torch.randn(*shape, generator=g) * 0.3)
    p0 = torch.zeros(*shape)

    def step(seed, offset, sr):
        p = p0.clone().to(DEV)
        m, v = O.QuantizedBuffer.zeros(shape, DEV), O.QuantizedBuffer.zeros(shape, DEV)
        ops.adamw_step_q8(p, gr.to(DEV), m.parts(), v.parts(), step=1, lr=1e-3, sr_state=sr, seed=seed, offset=offset)
        return m, v

    (m, v), (m2, v2), (m3, _), (mr, vr) = step(77, 4, True), step(77, 4, True), step(77, 8, True), step(77, 4, False)
    mf, vf = torch.zeros(*shape, device=DEV), torch.zeros(*shape, device=DEV)
    ops.adamw_step(p0.clone().to(DEV), gr.to(DEV), mf, vf, step=1, lr=1e-3)  # the float32 values that were quantized
    for name, qb, qb2, rne, x in (("exp_avg", m, m2, mr, mf), ("exp_avg_sq", v, v2, vr, vf)):
        assert torch.equal(qb.scale, rne.scale) and torch.equal(qb.zero_point, rne.zero_point)  # min and max carry no noise
        xg = x.cpu().double().view(256, 8, 32)
        q = (xg - qb.zero_point.cpu().double()) / qb.scale.cpu().double()
        code = qb.weight.cpu().double()
        assert bool(((code - q).abs() <= 0.5 + 0.1 * math.sqrt(48 * math.log(2)) + 1e-4).all()), name
        near = torch.round(q).clamp(0, 255)
        # P(code == k) for k = near - 1, near, near + 1 (further is < 1e-20): Phi of the distances to the rounding boundaries
        phi = lambda z: 0.5 * (1 + torch.erf(z / math.sqrt(2)))  # noqa: E731
        up, down = 1 - phi((near + 0.5 - q) / 0.1), phi((near - 0.5 - q) / 0.1)
        up, down = torch.where(near >= 255, torch.zeros_like(up), up), torch.where(near <= 0, torch.zeros_like(down), down)
        p_move = up + down
        moved = (code != near).double().sum().item()
        expect, sigma = p_move.sum().item(), (p_move * (1 - p_move)).sum().sqrt().item()
        e_err = near - q + up - down
        var_err = (up + down) - (up - down) ** 2
        n = q.numel()
        mean, mean_expect, mean_sigma = (code - q).mean().item(), e_err.mean().item(), var_err.sum().sqrt().item() / n
        print(f"stochastic uint8 {name}: moved {moved:.0f} expected {expect:.1f} +- {sigma:.1f}; mean error {mean:.3g} expected "
              f"{mean_expect:.3g} +- {mean_sigma:.3g}; round-to-nearest moved {(rne.weight.cpu().double() != near).sum().item():.0f}")
        assert expect > 1000  # the noise moves enough codes for the count to mean something
        assert abs(moved - expect) <= 4 * sigma, name
        assert abs(mean - mean_expect) <= 4 * mean_sigma, name
        assert torch.equal(qb.weight, qb2.weight), name
    assert not torch.equal(m.weight, m3.weight)


@pytest.mark.parametrize("quantized", [False, True], ids=["dense", "quantized"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_result_does_not_depend_on_launch_geometry(quantized, dtype):
    """One [130, 160] parameter and its two row halves [65, 160] as separate tensors (other grids, other block and wave boundaries, a
    start in the middle of the whole tensor's blocks): the same bits after two deterministic steps.  quantized_buffers_minimum_numel is
    lowered so that the halves (10 400 elements) get quantized state too."""
    O = _optim()
    g = torch.Generator().manual_seed(21)
    p0 = (torch.randn(130, 160, generator=g) * 0.5).to(dtype)
    grads = [(torch.randn(130, 160, generator=g) * 0.4).to(dtype) for _ in range(2)]
    kw = dict(lr=0.01, use_quantized_buffers=quantized, quantized_buffers_minimum_numel=4096, **OFF)
    whole = torch.nn.Parameter(p0.clone().to(DEV))
    halves = [torch.nn.Parameter(p0[:65].clone().to(DEV)), torch.nn.Parameter(p0[65:].clone().to(DEV))]
    oa, ob = O.AdamW([whole], **kw), O.AdamW(halves, **kw)
    for gr in grads:
        whole.grad = gr.clone().to(DEV)
        halves[0].grad, halves[1].grad = gr[:65].clone().to(DEV), gr[65:].clone().to(DEV)
        oa.step()
        ob.step()
    assert torch.equal(bits(whole.detach()), bits(torch.cat([h.detach() for h in halves])))
    for key in ("exp_avg", "exp_avg_sq"):
        a, b = oa.state[whole][key], [ob.state[h][key] for h in halves]
        assert isinstance(a, O.QuantizedBuffer) == quantized
        if quantized:
            for pa, pb0, pb1 in zip(a.parts(), b[0].parts(), b[1].parts()):
                assert torch.equal(bits(pa), bits(torch.cat([pb0, pb1])))
        else:
            assert torch.equal(bits(a), bits(torch.cat(b)))


@pytest.mark.parametrize("quantized", [False, True], ids=["dense", "quantized"])
def test_step_is_captured_in_a_graph_and_replays_the_eager_bits(quantized):
    """No host synchronisation: ``opt.step()`` itself is captured with torch.cuda.graph after an eager warm-up step (which creates the
    state), replayed once, and compared bit for bit with an eager optimizer taking the same two steps.  ``state["step"]`` is a Python int
    that ``step()`` advances while it is being captured, so the graph holds step 2's bias correction: one replay is step 2."""
    O = _optim()
    g = torch.Generator().manual_seed(31)
    p0 = (torch.randn(130, 160, generator=g) * 0.5).bfloat16()
    grads = [(torch.randn(130, 160, generator=g) * 0.4).bfloat16().to(DEV) for _ in range(2)]
    kw = dict(lr=0.01, use_quantized_buffers=quantized, **OFF)
    scale = torch.tensor(2.0, device=DEV)
    eager_p, graph_p = torch.nn.Parameter(p0.clone().to(DEV)), torch.nn.Parameter(p0.clone().to(DEV))
    eager, graphed = O.AdamW([eager_p], **kw), O.AdamW([graph_p], **kw)
    eager.grad_scale = graphed.grad_scale = scale
    for gr in grads:
        eager_p.grad = gr.clone()
        eager.step()
    graph_p.grad = grads[0].clone()
    graphed.step()
    graph_p.grad.copy_(grads[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    assert graphed.state[graph_p]["step"] == 2
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(graph_p.detach()), bits(eager_p.detach()))
    for key in ("exp_avg", "exp_avg_sq"):
        a, b = graphed.state[graph_p][key], eager.state[eager_p][key]
        for x, y in zip(a.parts() if quantized else (a,), b.parts() if quantized else (b,)):
            assert torch.equal(bits(x), bits(y))

@pytest.mark.parametrize("quantized", [False, True], ids=["dense", "quantized"])
def test_adamw_loop_trains_the_int8_linear(quantized):
    """Ten AdamW steps on a 64 -> 64 layer with 128 tokens through int8_matmul_dynamic_with_backward (the loop of
    test_sgd_loop_tracks_float32_linear): the loss falls below half its start and stays within 5 % of the same loop under
    torch.optim.AdamW, with the update clip disabled on both sides (clip_threshold large; torch has none).  A sanity check, not a
    precision claim.  Quantized state is forced for the 4096-element weight by quantized_buffers_minimum_numel."""
    from sdnq_amd import training as T
    O = _optim()

    def loop(make):
        g = torch.Generator().manual_seed(11)
        x = torch.randn(128, 64, generator=g).to(DEV)
        w = (torch.randn(64, 64, generator=g) * 0.1).to(DEV).requires_grad_(True)
        b = torch.zeros(64, device=DEV, requires_grad=True)
        target = (x @ (torch.randn(64, 64, generator=g) * 0.2).to(DEV) + 0.3).detach()
        opt = make([w, b])
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(T.int8_matmul_dynamic_with_backward(x, w, b), target)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return losses
    lr, wd, eps_free = 0.02, 0.01, 1e30
    mine = loop(lambda ps: O.AdamW(ps, lr=lr, weight_decay=wd, clip_threshold=(eps_free, 1e-3, 1e-3), use_quantized_buffers=quantized,
                                   quantized_buffers_minimum_numel=1024))
    ref = loop(lambda ps: torch.optim.AdamW(ps, lr=lr, weight_decay=wd, eps=0.0))
    print("losses", mine, ref)
    assert mine[-1] < 0.5 * mine[0]
    for a, r in zip(mine, ref):
        assert abs(a - r) <= 0.05 * r, (mine, ref)
