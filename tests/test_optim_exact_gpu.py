"""The fused AdamW step on the MI355X (csrc/optim.hip) against the float32 oracle (oracle/oracle.py: adamw_step, adamw_step_q8,
adamw_halves, stochastic_round_bits, stochastic_codes), which tests/test_optim_oracle.py pins to the reference's fixtures bit for bit.

State (dense exp_avg / exp_avg_sq; uint8 codes, scales, zero points) must have the oracle's BITS: every operation behind it is an IEEE
operation in a fixed order.  The parameter alone sees the device's rsqrt (1 ulp, where the oracle computes 1 / sqrt, 1 ulp too), so it
follows the PARAMETER RULE: with tol_i = lr |u_i| 2^-21 + ulp32(p_i) from the oracle's update u and float32 p -- u differs by less than
3 * 2^-23 relative (the two rsqrt and two product roundings), and the final fma rounds once on each side -- a float32 parameter lies in
[p - tol, p + tol], a 16-bit one in [store(p - tol), store(p + tol)], store being the deterministic rounding or the stochastic one with
the predicted bits (both monotone).  Where |u| in front of its clamp exceeds the clip by more than that 2^-20, both sides sit on the
bound and tol is 0.  Two conditions come from the oracle alone: at most 1 % of the 16-bit elements may have two different endpoint
roundings, and a clamped element admits one value only.  What was measured: profiles/optim_adamw_accuracy.md."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as U  # noqa: E402
from test_optim_gpu import fixture_optimizer  # noqa: E402

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAGS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL, FRONT, BACK = 0xA5, 64, 256
BIG = (0x123456789ABCDEF0, (1 << 32) + 12)  # (seed, offset): both above 2^32
SMALL = (7, 3)
AMBIGUOUS_CAP, EXCLUDED_CAP, MARGIN = 0.01, 0.005, 2.0 ** -10


def _ops():
    from sdnq_amd import ops
    return ops


class Tally:
    """Counts over one test: 16-bit elements whose two endpoint roundings differ, and the largest float32 distance in units of tol."""

    def __init__(self):
        self.ambiguous = self.total = 0
        self.dist = 0.0

    def share(self):
        return self.ambiguous / max(self.total, 1)


def param_rule(got, r, tag, lr, clip, tally, halves=None, what=""):
    """Assert the parameter rule for `got` (a tensor of dtype `tag`) against the oracle's result `r` of the same step."""
    p = r["p"].astype(np.float64)
    ulp = np.spacing(np.minimum(np.abs(r["p"]), np.float32(2.0 ** 127)))  # the top binade's ulp from its start: spacing(max) overflows
    tol = lr * np.abs(r["u"].astype(np.float64)) * 2.0 ** -21 + ulp.astype(np.float64)
    tol[np.abs(r["u_raw"].astype(np.float64)) >= clip * (1.0 + 2.0 ** -20)] = 0.0
    with np.errstate(over="ignore"):  # an endpoint past the largest float32 becomes an infinity: no bound on that side
        lo, hi = (p - tol).astype(np.float32), (p + tol).astype(np.float32)
    g = U.f32_array(got)
    assert g.shape == lo.shape, what
    if tag == "f32":
        bad = np.flatnonzero(~((g >= lo) & (g <= hi)) | ((tol == 0) & (g.view(np.uint32) != r["p"].view(np.uint32))))
        assert bad.size == 0, (what, "parameter", bad[:8].tolist(), g[bad[:8]].tolist(), r["p"][bad[:8]].tolist())
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(tol > 0, np.abs(g.astype(np.float64) - p) / tol, 0.0)
        tally.dist = max(tally.dist, float(d.max()))
        return
    store = (lambda x: O.round_dtype(x, tag)) if halves is None else (lambda x: O.stochastic_round_bits(x, halves, tag))
    slo, shi = store(lo), store(hi)
    one = U.stored_bits(slo, tag) == U.stored_bits(shi, tag)
    tally.ambiguous += int((~one).sum())
    tally.total += one.size
    assert not (~one & (tol == 0)).any(), what  # a clamped element admits one value
    ok = np.where(one, U.bit_array(got) == U.stored_bits(slo, tag), (g >= slo) & (g <= shi))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (what, "parameter", bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), slo[bad[:8]].tolist(), shi[bad[:8]].tolist())


def same_bits(got, want_bits, what):
    g = U.bit_array(got)
    assert g.dtype == want_bits.dtype and g.shape == want_bits.shape, what
    bad = np.flatnonzero(g != want_bits)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), (bad[:8] % 8).tolist(), g[bad[:8]].tolist(), want_bits[bad[:8]].tolist())


class Guarded:
    """A tensor of the given values in the middle of a larger allocation filled with a sentinel byte; its start is 16-byte aligned."""

    def __init__(self, values):
        self.nbytes = values.numel() * values.element_size()
        self.buf = torch.full((FRONT + self.nbytes + BACK,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.buf[FRONT:FRONT + self.nbytes].view(values.dtype)
        self.t.copy_(values.reshape(-1))
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:FRONT] == SENTINEL).all()) and bool((self.buf[FRONT + self.nbytes:] == SENTINEL).all())


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.names())
def test_fixture_state_is_bit_equal_and_the_parameter_follows_the_rule(name):
    """Each of the fixture's three steps through the public AdamW, started from the fixture's state in front of it: dense state and
    uint8 codes, scales and zero points have the fixture's bits (which are the oracle's: tests/test_optim_oracle.py); the parameter
    follows the parameter rule."""
    meta, t = U.load(name)
    tag, tally = meta["dtype"], Tally()
    for i in range(1, U.STEPS + 1):
        r = U.oracle_fixture_step(name, i)
        opt, p = fixture_optimizer(name, i)
        opt.step()
        st = opt.state[p]
        kw = U.oracle_options(meta, i)
        for key in ("exp_avg", "exp_avg_sq"):
            parts = dict(zip(("_q", "_scale", "_zp"), st[key].parts())) if meta["quantized"] else {"": st[key]}
            for part, got in parts.items():
                assert got.shape == t[f"{key}{part}{i}"].shape
                same = (U.bit_array(got) == U.bit_array(t[f"{key}{part}{i}"])).mean()
                print(f"exact {name} step {i} {key}{part}: bit-equal to the fixture {same:.6f}")
                same_bits(got, U.bit_array(t[f"{key}{part}{i}"]), (name, i, key + part))
        same = (U.bit_array(p.detach()) == U.bit_array(t[f"p{i}"])).mean()
        before = tally.ambiguous
        param_rule(p.detach(), r, tag, kw["lr"], kw["clip"], tally, what=(name, i))
        print(f"exact {name} step {i} p: bit-equal to the fixture {same:.6f}, interval-ambiguous {tally.ambiguous - before}, "
              f"largest float32 distance so far {tally.dist:.3f} tol")
    if tag != "f32":
        print(f"exact {name}: interval-ambiguous share {tally.share():.6f}")
        assert tally.share() <= AMBIGUOUS_CAP


# ---- size sweep --------------------------------------------------------------------------------------------------------------------------
DENSE_SIZES = [1, 2, 7, 8, 9, 15, 16, 63, 64, 65, 511, 512, 513, 2040, 2047, 2048, 2049, 2055, 4095, 4096, 4097, 6151]
Q8_SIZES = [32, 64, 96, 2016, 2048, 2080, 4064, 4096, 4128, 20800]


def _config(k):
    """The options of the k-th size of a sweep: both beta pairs, weight decay 0 and not, clip 1 and 0.25 -- every pair of the three
    switches occurs within eight consecutive sizes."""
    return dict(lr=0.02, betas=(0.9, 0.999) if k % 2 == 0 else (0.4, 0.3), weight_decay=0.0 if (k // 2) % 2 == 0 else 0.1,
                clip=1.0 if (k // 4) % 2 == 0 else 0.25)


def _plant(x, values, n):
    """`values` = (at index 0, at the last index, at the start of the tail n - n % 8 when there is one) into the flat tensor x."""
    x[0], x[n - 1] = values[0], values[1]
    if n % 8 and n - n % 8 not in (0, n - 1):
        x[n - n % 8] = values[2]


@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
def test_size_sweep_dense_state(tag):
    """Two consecutive deterministic steps through ops.adamw_step at sizes around the lane (8), wave (512) and block (2048) boundaries,
    with a grad_scale tensor and special values at the first, the last and the first tail element; every tensor inside a sentinel-filled
    allocation.  State: the oracle's bits; parameter: the parameter rule; sentinels untouched.  Odd sizes of the list start from a random
    state at step 5, even ones from zeros at step 1."""
    ops, dt, tally = _ops(), TAGS[tag], Tally()
    top, tiny = torch.finfo(dt).max, {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}[tag]
    gs = torch.tensor([3.0], dtype=torch.float32, device=DEV)
    for k, n in enumerate(DENSE_SIZES):
        g = torch.Generator().manual_seed(1000 + n)
        kw = _config(k)
        p0 = torch.randn(n, generator=g) * 0.5
        _plant(p0, (float("-inf"), float("nan"), top), n)
        first = 5 if k % 2 else 1
        m0 = torch.randn(n, generator=g) * 0.1 if k % 2 else torch.zeros(n)
        v0 = torch.rand(n, generator=g) * 0.1 if k % 2 else torch.zeros(n)
        P, M, V = Guarded(p0.to(dt)), Guarded(m0.to(dt)), Guarded(v0.to(dt))
        for step in (first, first + 1):
            gr = torch.randn(n, generator=g) * 1.5
            _plant(gr, (float("nan"), float("inf"), tiny) if step == first else (tiny, float("-inf"), 0.0), n)
            G = Guarded(gr.to(dt))
            r = O.adamw_step(U.f32_array(P.t), U.f32_array(G.t), U.f32_array(M.t), U.f32_array(V.t), tag, step=step, grad_scale=3.0, **kw)
            ops.adamw_step(P.t, G.t, M.t, V.t, step=step, grad_scale=gs, **kw)
            torch.cuda.synchronize()
            what = (tag, n, step)
            assert P.intact() and G.intact() and M.intact() and V.intact(), what
            same_bits(M.t, U.stored_bits(r["exp_avg"], tag), what + ("exp_avg",))
            same_bits(V.t, U.stored_bits(r["exp_avg_sq"], tag), what + ("exp_avg_sq",))
            param_rule(P.t, r, tag, kw["lr"], kw["clip"], tally, what=what)
    print(f"exact sweep dense {tag}: interval-ambiguous share {tally.share():.6f}, largest float32 distance {tally.dist:.3f} tol")
    assert tally.share() <= AMBIGUOUS_CAP


def test_size_sweep_uint8_state():
    """The same through ops.adamw_step_q8 at sizes around the block boundaries (whole groups of 32), the parameter's dtype cycling
    through the three; the second step starts from the first step's codes.  One group of gradients is all zero (scale 0, codes 0)."""
    ops, tally = _ops(), Tally()
    gs = torch.tensor([3.0], dtype=torch.float32, device=DEV)
    for k, n in enumerate(Q8_SIZES):
        tag = ("f32", "bf16", "f16")[k % 3]
        dt = TAGS[tag]
        g = torch.Generator().manual_seed(2000 + n)
        kw = _config(k)
        p0 = torch.randn(n, generator=g) * 0.5
        _plant(p0, (float("-inf"), float("nan"), 0.0), n)
        P = Guarded(p0.to(dt))
        state = [[Guarded(torch.zeros(n, dtype=torch.uint8)), Guarded(torch.zeros(n // 32)), Guarded(torch.zeros(n // 32))] for _ in range(2)]
        for step in (1, 2):
            gr = torch.randn(n, generator=g) * 1.5
            _plant(gr, (float("nan"), float("inf"), 0.0), n)
            if n >= 96:
                gr[32:64] = 0.0
            G = Guarded(gr.to(dt))
            before = [tuple(x.t.cpu().numpy() for x in s) for s in state]
            r = O.adamw_step_q8(U.f32_array(P.t), U.f32_array(G.t), before[0], before[1], tag, step=step, grad_scale=3.0, **kw)
            ops.adamw_step_q8(P.t, G.t, tuple(x.t for x in state[0]), tuple(x.t for x in state[1]), step=step, grad_scale=gs, **kw)
            torch.cuda.synchronize()
            what = (tag, n, step)
            assert P.intact() and G.intact() and all(x.intact() for s in state for x in s), what
            for key, s in zip(("exp_avg", "exp_avg_sq"), state):
                same_bits(s[1].t, r[key + "_scale"].view(np.uint32), what + (key, "scale"))
                same_bits(s[2].t, r[key + "_zp"].view(np.uint32), what + (key, "zero point"))
                same_bits(s[0].t, r[key + "_q"], what + (key, "codes"))
            if n >= 96:
                assert float(state[0][1].t[1]) == 0 and int(state[0][0].t[32:64].max()) == 0
            param_rule(P.t, r, tag, kw["lr"], kw["clip"], tally, what=what)
    print(f"exact sweep uint8: interval-ambiguous share {tally.share():.6f}, largest float32 distance {tally.dist:.3f} tol")
    assert tally.share() <= AMBIGUOUS_CAP


# ---- stochastic rounding, predicted ------------------------------------------------------------------------------------------------------
def _inputs(n, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(n, generator=g) * 0.5).to(dt), (torch.randn(n, generator=g) * 0.4).to(dt),
            (torch.randn(n, generator=g) * 0.1).to(dt), (torch.rand(n, generator=g) * 0.1).to(dt))


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_stochastic_rounding_uses_the_predicted_bits(tag):
    """Dense state: one step from a random state with every combination of the two switches, a (seed, offset) above 2^32 and a small
    one, a size with a tail and one of 32 blocks.  A stochastically stored state tensor equals stochastic_round_bits(the oracle's float32
    value, the predicted half word of its stream), a deterministic one the ordinary rounding; the parameter follows the rule with the
    bits of stream 0."""
    ops, dt, tally = _ops(), TAGS[tag], Tally()
    kw = dict(step=4, lr=0.02, betas=(0.9, 0.999), weight_decay=0.01, clip=1.0)
    for n in (2055, 65536):
        p0, gr, m0, v0 = _inputs(n, dt, 40 + n)
        r = O.adamw_step(U.f32_array(p0), U.f32_array(gr), U.f32_array(m0), U.f32_array(v0), tag, **kw)
        for seed, offset in (BIG, SMALL):
            halves = [O.adamw_halves(n, seed, offset, s) for s in (0, 1, 2)]
            for sr_param, sr_state in ((True, False), (False, True), (True, True)):
                p, m, v = p0.clone().to(DEV), m0.clone().to(DEV), v0.clone().to(DEV)
                ops.adamw_step(p, gr.to(DEV), m, v, sr_param=sr_param, sr_state=sr_state, seed=seed, offset=offset, **kw)
                what = (tag, n, seed, offset, sr_param, sr_state)
                for key, got, h in (("exp_avg", m, halves[1]), ("exp_avg_sq", v, halves[2])):
                    want = O.stochastic_round_bits(r[key], h, tag) if sr_state else O.round_dtype(r[key], tag)
                    same_bits(got, U.stored_bits(want, tag), what + (key,))
                param_rule(p, r, tag, kw["lr"], kw["clip"], tally, halves=halves[0] if sr_param else None, what=what)
    print(f"exact stochastic dense {tag}: interval-ambiguous share {tally.share():.6f}")
    assert tally.share() <= AMBIGUOUS_CAP


def _check_codes(qb_parts, x, seed, offset, streams, what):
    """uint8 state stored stochastically against stochastic_codes of the oracle's float32 state `x`; returns the excluded share."""
    code, scale, zp, margin = O.stochastic_codes(x, seed, offset, streams)
    excluded = margin <= MARGIN
    share = float(excluded.mean())
    assert share <= EXCLUDED_CAP, (what, share)  # from the oracle alone
    same_bits(qb_parts[1], scale.view(np.uint32), what + ("scale",))  # min and max carry no noise
    same_bits(qb_parts[2], zp.view(np.uint32), what + ("zero point",))
    got = U.bit_array(qb_parts[0]).astype(np.int64)
    bad = np.flatnonzero(np.where(excluded, np.abs(got - code) > 1, got != code))
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), code[bad[:8]].tolist(), margin[bad[:8]].tolist())
    return share, float((got != code).mean())


def test_stochastic_uint8_state_uses_the_predicted_normals():
    """uint8 state with sr_state: scale and zero point have the deterministic oracle's bits; every code equals the oracle's
    round(q + 0.1 z), z from Box-Muller in double on the predicted words, wherever q + 0.1 z lies more than 2^-10 from a rounding
    boundary -- an error of 0.01 in a device normal, orders above what the hardware's log, sin and cos leave -- and is one of the two
    neighbours inside that margin.  Inputs: those of test_stochastic_rounding_of_a_uint8_buffer (float32 [256, 256], seed 77, offset 4),
    where the oracle alone excludes 0.16 % of either buffer's codes, and a bf16 parameter stored stochastically too, with a (seed, offset) above 2^32."""
    from sdnq_amd import optim
    ops = _ops()
    n = 256 * 256
    g = torch.Generator().manual_seed(9)
    gr32 = torch.randn(256, 256, generator=g) * 0.3
    for tag, p0, gr, (seed, offset), sr_param in (("f32", torch.zeros(256, 256), gr32, (77, 4), False),
                                                  ("bf16", _inputs(n, torch.bfloat16, 3)[0].view(256, 256), gr32.bfloat16(), BIG, True)):
        tally = Tally()
        kw = dict(step=1, lr=1e-3)
        zeros = (np.zeros(n, dtype=np.uint8), np.zeros(n // 32, dtype=np.float32), np.zeros(n // 32, dtype=np.float32))
        r = O.adamw_step_q8(U.f32_array(p0), U.f32_array(gr), zeros, zeros, tag, **kw)
        p = p0.clone().to(DEV)
        m, v = optim.QuantizedBuffer.zeros((256, 256), DEV), optim.QuantizedBuffer.zeros((256, 256), DEV)
        ops.adamw_step_q8(p, gr.to(DEV), m.parts(), v.parts(), sr_param=sr_param, sr_state=True, seed=seed, offset=offset, **kw)
        for key, qb, streams in (("exp_avg", m, (1, 3)), ("exp_avg_sq", v, (2, 4))):
            share, moved = _check_codes(qb.parts(), r[key], seed, offset, streams, (tag, key))
            print(f"exact stochastic uint8 {tag} {key}: Box-Muller excluded share {share:.6f}, codes off the oracle's {moved:.6f}")
        param_rule(p, r, tag, kw["lr"], 1.0, tally, halves=O.adamw_halves(n, seed, offset, 0) if sr_param else None, what=(tag, "p"))
        print(f"exact stochastic uint8 {tag} p: interval-ambiguous share {tally.share():.6f}, float32 distance {tally.dist:.3f} tol")
        assert tally.share() <= AMBIGUOUS_CAP


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_stochastic_parameter_with_deterministic_uint8_state(tag):
    """A 16-bit parameter with uint8 state, sr_param alone: the parameter follows the rule with the bits of stream 0, the state has the
    deterministic oracle's bits."""
    ops, dt, tally = _ops(), TAGS[tag], Tally()
    kw = dict(step=1, lr=0.02, betas=(0.4, 0.3), clip=0.25)
    for n, (seed, offset) in ((2080, BIG), (20800, SMALL)):
        p0, gr, _, _ = _inputs(n, dt, 60 + n)
        zeros = (np.zeros(n, dtype=np.uint8), np.zeros(n // 32, dtype=np.float32), np.zeros(n // 32, dtype=np.float32))
        r = O.adamw_step_q8(U.f32_array(p0), U.f32_array(gr), zeros, zeros, tag, **kw)
        p = p0.clone().to(DEV)
        state = [(torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n // 32, device=DEV), torch.zeros(n // 32, device=DEV)) for _ in range(2)]
        ops.adamw_step_q8(p, gr.to(DEV), state[0], state[1], sr_param=True, sr_state=False, seed=seed, offset=offset, **kw)
        for key, s in zip(("exp_avg", "exp_avg_sq"), state):
            same_bits(s[0], r[key + "_q"], (tag, n, key, "codes"))
            same_bits(s[1], r[key + "_scale"].view(np.uint32), (tag, n, key, "scale"))
            same_bits(s[2], r[key + "_zp"].view(np.uint32), (tag, n, key, "zero point"))
        param_rule(p, r, tag, kw["lr"], kw["clip"], tally, halves=O.adamw_halves(n, seed, offset, 0), what=(tag, n))
    print(f"exact stochastic parameter, uint8 state {tag}: interval-ambiguous share {tally.share():.6f}")
    assert tally.share() <= AMBIGUOUS_CAP


# ---- the optimizer's draw ------------------------------------------------------------------------------------------------------------------
def test_optimizer_hands_out_seed_and_offsets_and_advances_the_generator():
    """SDNQOptimizer.step reads (seed, offset) from torch's device generator once; the i-th tensor that needs random bits uses
    offset + i (a float32 tensor with dense state draws nothing and does not count); the generator moves on by the count rounded up to a
    multiple of 4.  Predicted with the oracle for two steps; the same seed and a fresh optimizer repeat the first run's bits."""
    from sdnq_amd import optim
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    shapes = [("bf16", (37, 24)), ("f32", (37, 24)), ("bf16", (83,))]
    g = torch.Generator().manual_seed(17)
    p0 = [(torch.randn(*s, generator=g) * 0.5).to(TAGS[t]) for t, s in shapes]
    grads = [[(torch.randn(*s, generator=g) * 0.4).to(TAGS[t]) for t, s in shapes] for _ in range(2)]

    def run():
        torch.cuda.manual_seed(1234)
        params = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
        opt = optim.AdamW(params)
        group = opt.param_groups[0]
        assert group["use_stochastic_rounding"] is True and group["use_stochastic_buffers"] is True
        tally, snapshots = Tally(), []
        for i, grs in enumerate(grads, 1):
            o = gen.get_offset()
            before = [(U.f32_array(p), *((U.f32_array(opt.state[p][k]) for k in ("exp_avg", "exp_avg_sq")) if i > 1 else
                                        (np.zeros(p.numel(), dtype=np.float32),) * 2)) for p in params]
            for p, gr in zip(params, grs):
                p.grad = gr.clone().to(DEV)
            opt.step()
            assert gen.initial_seed() == 1234 and gen.get_offset() == o + 4
            used = 0
            for (tag, _), p, gr, (pb, mb, vb) in zip(shapes, params, grs, before):
                r = O.adamw_step(pb, U.f32_array(gr), mb, vb, tag, step=i, lr=group["lr"], betas=group["betas"],
                                 weight_decay=group["weight_decay"], clip=group["clip_threshold"][0])
                halves = [None] * 3
                if tag != "f32":
                    halves = [O.adamw_halves(p.numel(), 1234, o + used, s) for s in (0, 1, 2)]
                    used += 1
                for key, h in (("exp_avg", halves[1]), ("exp_avg_sq", halves[2])):
                    want = r[key] if h is None else O.stochastic_round_bits(r[key], h, tag)
                    same_bits(opt.state[p][key], U.stored_bits(want, tag), (i, tag, key))
                param_rule(p.detach(), r, tag, group["lr"], group["clip_threshold"][0], tally, halves=halves[0], what=(i, tag))
            assert used == 2
            snapshots.append([U.bit_array(x).copy() for p in params for x in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])])
        assert tally.share() <= AMBIGUOUS_CAP
        return snapshots

    first, again = run(), run()
    for a, b in zip(first[0] + first[1], again[0] + again[1]):
        assert (a == b).all()
