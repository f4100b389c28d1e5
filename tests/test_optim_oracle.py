"""The float32 oracle of the AdamW step (oracle/sdnq_oracle.c: orc_adamw_step, orc_adamw_step_q8, orc_philox4x32_10,
orc_stochastic_codes; oracle/oracle.py) against what pins it: the reference's fixtures tests/golden/optim_adamw_* bit for bit, the
published Philox4x32-10 known answers, and the reference's stochastic-rounding formula evaluated in torch on the same integers.  No GPU:
tests/test_optim_exact_gpu.py then holds the kernel to this oracle."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as U  # noqa: E402

from oracle import oracle as O  # noqa: E402


@pytest.mark.parametrize("name", U.names())
def test_oracle_reproduces_the_fixture_bit_for_bit(name):
    """Every tensor the reference left after each of the three steps, each step started from the fixture's own state in front of it:
    the oracle's float32 result, rounded to the storage dtype, has the same bits (-0.0 is not 0.0)."""
    meta, t = U.load(name)
    tag = meta["dtype"]
    for i in range(1, U.STEPS + 1):
        r = U.oracle_fixture_step(name, i)
        pairs = [("p", U.stored_bits(r["p"], tag))]
        for key in ("exp_avg", "exp_avg_sq"):
            if meta["quantized"]:
                pairs += [(key + "_q", r[key + "_q"]), (key + "_scale", r[key + "_scale"].view(np.uint32)), (key + "_zp", r[key + "_zp"].view(np.uint32))]
            else:
                pairs.append((key, U.stored_bits(r[key], tag)))
        for key, got in pairs:
            want = U.bit_array(t[f"{key}{i}"])
            assert got.dtype == want.dtype and got.shape == want.shape, (key, i)
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (name, i, key, diff.size, diff[:8].tolist())
        for key in ("p", "exp_avg", "exp_avg_sq", "u"):
            assert np.isfinite(r[key]).all(), (name, i, key)


def test_fixtures_hold_no_non_finite_result_and_reach_both_lerp_branches():
    """What the fixtures are for: no stored result is non-finite (optim_util.distance would mean nothing), and the set has 1 - beta on
    both sides of 0.5, a clip below 1 and special values planted in a parameter."""
    small = big = low_clip = param_plants = False
    for name in U.names():
        meta, t = U.load(name)
        for key, x in t.items():
            if key not in ("p0", "g1", "g2", "g3") and x.is_floating_point():
                assert bool(torch.isfinite(x.float()).all()), (name, key)
        for b in meta["options"]["betas"]:
            small, big = small or 1 - b < 0.5, big or 1 - b >= 0.5
        low_clip = low_clip or meta["options"]["clip_threshold"][0] < 1
        if meta.get("planted_param"):
            param_plants = True
            flat = t["p0"].view(-1).float()
            kinds = {what: flat[int(i)] for i, what in meta["planted_param"].items()}
            assert torch.isnan(kinds["nan"]) and kinds["inf"] == float("inf") and kinds["-inf"] == -float("inf")
            assert kinds["-0.0"] == 0 and torch.signbit(kinds["-0.0"]) and 0 < kinds["tiny"] < torch.finfo(t["p0"].dtype).smallest_normal
            assert kinds["max"] == torch.finfo(t["p0"].dtype).max == -kinds["-max"]
    assert small and big and low_clip and param_plants


KNOWN = [  # counter; key -> words (Random123's known-answer vectors for philox4x32 with 10 rounds)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_known_answers():
    for counter, key, words in KNOWN:
        assert O.philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32)).tolist() == list(words)
    # vectorised over counters: every row is its own call
    many = O.philox4x32_10(np.array([k[0] for k in KNOWN[::2]] * 3, dtype=np.uint32), np.array(KNOWN[0][1], dtype=np.uint32))
    assert many.shape == (6, 4) and many[0].tolist() == list(KNOWN[0][2]) and (many[0] == many[2]).all() and (many[1] == many[3]).all()


def test_words_follow_the_counter_layout():
    """adamw_words / adamw_halves: counter (e8 low, e8 high | stream << 28, offset low, offset high), key (seed low, seed high);
    element e of eight takes half e & 1 of word e >> 1."""
    seed, offset = 0x123456789ABCDEF0, (1 << 32) + 12
    w = O.adamw_words(20, seed, offset, 2)
    assert w.shape == (3, 4)
    one = O.philox4x32_10(np.array([2, 2 << 28, 12, 1], dtype=np.uint32), np.array([0x9ABCDEF0, 0x12345678], dtype=np.uint32))
    assert w[2].tolist() == one.tolist()
    h = O.adamw_halves(20, seed, offset, 2)
    assert h.shape == (20,) and int(h[16]) == int(one[0]) & 0xFFFF and int(h[17]) == int(one[0]) >> 16 and int(h[19]) == int(one[1]) >> 16
    # seed_hi, off_hi and the stream all reach the words
    for other in (O.adamw_words(20, seed & 0xFFFFFFFF, offset, 2), O.adamw_words(20, seed, 12, 2), O.adamw_words(20, seed, offset, 1)):
        assert not (other == w).any(axis=1).all()


SR = {"bf16": (torch.bfloat16, 1 << 16), "f16": (torch.float16, 1 << 13)}


def _sr_inputs(tag):
    dt, step = SR[tag]
    g = torch.Generator().manual_seed(5 + step)
    top = torch.finfo(dt).max
    rand = torch.randn(4096, generator=g) * torch.tensor([1e-3, 1.0, 300.0, 6e4]).repeat(1024)         # both signs, several binades
    grid = (torch.randn(512, generator=g) * 3).to(dt).float()                                            # exactly on the 16-bit grid
    below = torch.tensor([top, -top]).view(torch.int32).sub(1).view(torch.float32).repeat(256)           # one float32 ulp below the max
    sub = torch.cat([torch.rand(512, generator=g) * 6.2e-5, -torch.rand(512, generator=g) * 6.2e-5,      # float16 subnormals
                     torch.tensor([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, -(2.0 ** -25), 0.0, -0.0])])
    inf = torch.tensor([float("inf"), -float("inf")]).repeat(64)
    x = torch.cat([rand, grid, below, sub, inf])
    r = torch.randint(0, 1 << 16, (x.numel(),), generator=g, dtype=torch.int32)
    r[:8] = torch.tensor([0, step - 1, step, 0xFFFF, 1, step // 2, step // 2 - 1, 0x8000])
    return x, r


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_stochastic_round_bits_equals_the_reference_formula(tag):
    """copy_stochastic_ (optim/utils.py) with its randint replaced by given integers below `step`, in torch on the CPU:
    (r + x.view(int32)) & -step, viewed as float32, clamped to the dtype's finite range, .to(dtype).  The oracle takes 16 random bits
    and masks them itself."""
    dt, step = SR[tag]
    x, r = _sr_inputs(tag)
    top = torch.finfo(dt).max
    want = (r & (step - 1)).add(x.view(torch.int32)).bitwise_and_(-step).view(torch.float32).clamp_(-top, top).to(dt)
    got = O.stochastic_round_bits(x.numpy(), r.numpy().astype(np.uint32), tag)
    assert (U.stored_bits(got, tag) == U.bit_array(want)).all()
    assert (O.round_dtype(got, tag).view(np.uint32) == got.view(np.uint32)).all()  # already values of the dtype
    assert np.isfinite(got).all()                                                   # +-inf were clamped
    if tag == "f16":  # the ordinary rounding did move some subnormals: the masked float32 value was not a float16 yet
        masked = (r & (step - 1)).add(x.view(torch.int32)).bitwise_and_(-step).view(torch.float32)
        assert bool((masked != want.float()).any())
    nan = O.stochastic_round_bits(np.array([np.nan], dtype=np.float32), np.array([3], dtype=np.uint32), tag)
    assert np.isnan(nan).all()


def test_stochastic_codes_without_noise_words_and_margins():
    """orc_stochastic_codes on hand-made words: u1 = 1 (word 0xFFFFFF00 and above) makes sqrt(-2 ln u1) = 0, so z = 0 and the codes
    are the deterministic ones; the margin is the distance of q from the nearest k + 0.5; an all-equal group has scale 0, codes 0."""
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(96, generator=g) * 0.2).numpy()
    x[32:64] = 0.25
    w = np.full((12, 8), 0xFFFFFFFF, dtype=np.uint32)
    code, margin = np.empty(96, dtype=np.uint8), np.empty(96)
    scale, zp = np.empty(3, dtype=np.float32), np.empty(3, dtype=np.float32)
    assert O.lib().orc_stochastic_codes(O._p(x), O._p(w), 96, O._p(code), O._p(scale), O._p(zp), O._p(margin)) == 0
    zero = np.zeros(96, dtype=np.float32)
    st = (np.zeros(96, dtype=np.uint8), np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    # the deterministic quantizer of adamw_step_q8 on the same values: w1 = 1 makes exp_avg the gradient itself
    det = O.adamw_step_q8(zero, x, st, st, "f32", step=1, lr=0.0, betas=(0.0, 0.5), weight_decay=0.0, clip=10.0)
    assert (det["exp_avg"] == x).all() and (det["exp_avg_q"] == code).all()
    assert (det["exp_avg_scale"] == scale).all() and (det["exp_avg_zp"] == zp).all()
    assert scale[1] == 0 and (code[32:64] == 0).all() and (margin[32:64] == 1).all()
    with np.errstate(invalid="ignore"):
        q = (x.astype(np.float32) - np.repeat(zp, 32)) / np.repeat(scale, 32)
    inner = (q > 0) & (q < 255)
    inner[32:64] = False
    assert np.allclose(margin[inner], np.abs(q[inner] - np.floor(q[inner]) - 0.5), atol=1e-12) and (margin[~inner] == 1).all()
    # real words: every code within 0.5 + 0.1 * 5.77 of q, some moved, min and max untouched
    code2, scale2, zp2, margin2 = O.stochastic_codes(x, 77, 4, (1, 3))
    assert (scale2 == scale).all() and (zp2 == zp).all() and (np.abs(code2[inner].astype(np.float64) - q[inner]) <= 0.5 + 0.578).all()
    assert (code2 != code).any() and (code2[32:64] == 0).all()
