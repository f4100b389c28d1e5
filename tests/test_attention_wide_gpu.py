"""Quantized attention forward for head dims 136 .. 256 (sdnq_amd/csrc/attention_wide.hip behind sdnq_hip_atten).

1. Against a float64 restatement of the reference's arithmetic (`restate`; triton_atten.py:443-487 and :143-335).  Only the kernel's own
   roundings separate the two.  With p_j the softmax weights normalised to their row maximum (l = sum p_j >= 1), u the unit roundoff of the
   value dtype (2^-8 bfloat16, 2^-11 float16), A = sum_j p_j |v_j| / l and L the largest |logit| (base 2) of the case:
     P is rounded to the value dtype, |rnd(p_j) - p_j| <= u p_j                                            -> u A
       (float16 only: a weight below 2^-14 is rounded with the absolute error 2^-25 of a subnormal           -> 2^-25 sum_j |v_j| / l)
     the output is rounded to its dtype                                                                      -> u |out|
     float32: the kn products of P.V and the kn terms of l are each added with a relative error 2^-24         -> 2 kn 2^-24 A
       a logit is ((acc * k_scale) * (q_scale * (sm_scale * log2 e))) [+ mask] - m: the two scales (amax / 127), sm_scale, log2 e, their
       three products, the mask and the subtraction are nine roundings, so a logit errs by at most 9 2^-24 L and a weight and its row sum
       by ln 2 times that each (2 ln 2 * 9 < 16), plus the ulps of exp2 and 1 / l: (16 L + 16) 2^-24 relative -> (16 L + 16) 2^-24 A
       (the scores themselves are exact integers below 2^24)
   together |got - out| <= u (A + |out|) + (2 kn + 16 L + 16) 2^-24 (A + |out|) [+ 2^-25 sum_j |v_j| / l].
   A code on a rounding tie may legitimately differ, so the inputs are built with no x / scale within 1e-3 of a half-integer (`off_ties`).
2. Planted key, bit for bit: integer Q and K with a +-127 in every token (every scale is exactly 1), one key 32258 score units above the
   rest (softmax exactly one-hot in float32), V distinct per (key, channel): the output is the planted key's V row at every channel.
3. What the host refuses."""
import functools
import math

import pytest
import torch

from sdnq_amd import _lib
from sdnq_amd.attention import sdnq_hip_atten

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
# (head dim, dtype, queries, keys, form): every DP with a ragged key tail, every q_len / kv_len and every form at least once; 300 keys
# take the two-launch prepare pass (channel sums first), the causal cases walk 0, 1 and 2 plain blocks in front of the diagonal
CASES = [(136, "bf16", 70, 97, "plain"), (160, "f16", 33, 161, "causal"), (192, "bf16", 70, 300, "bool"), (224, "f16", 33, 31, "float"),
         (256, "bf16", 70, 161, "gqa"), (160, "bf16", 70, 300, "token_major"), (224, "bf16", 1, 97, "no_smooth"), (256, "f16", 33, 1, "plain"),
         (192, "f16", 70, 300, "scale"), (256, "f16", 70, 161, "causal")]


def off_ties(x, smooth, gen):
    """Redraw, until none is left, the elements whose code x / scale lies within 1e-3 of a half-integer."""
    for _ in range(200):
        y = x.double()
        y = y - y.mean(2, keepdim=True) if smooth else y
        c = y / (y.abs().amax(-1, keepdim=True) / 127)
        bad = ((c - c.floor()) - 0.5).abs() < 1e-3
        if not bad.any():
            return x
        x = torch.where(bad, torch.randn(x.shape, generator=gen).to(x.dtype), x)
    raise AssertionError("the inputs did not settle off the rounding ties")


def restate(q, k, v, mask, causal, sm_scale, smooth):
    """float64: (out, A = sum p |v| / l, sum |v| / l, largest |logit|) of [Z, H, N, D] tensors; mask None, bool or additive (base-2 logits)."""
    q, k, v = q.double(), k.double(), v.double()
    if smooth:
        k = k - k.mean(2, keepdim=True)
    rep = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)  # kv head = h * kv_heads // q_heads
    qs, ks = q.abs().amax(-1, keepdim=True) / 127, k.abs().amax(-1, keepdim=True) / 127
    kc = torch.nan_to_num(torch.round(k / ks))  # a zero row (one key minus its own mean) has scale 0 and the codes 0, as in the kernels
    logits = (torch.round(q / qs) @ kc.transpose(-1, -2)) * qs * ks.transpose(-1, -2) * (sm_scale * math.log2(math.e))
    if mask is not None:
        logits = logits.masked_fill(~mask, -math.inf) if mask.dtype == torch.bool else logits + mask.double()
    if causal:  # aligned top-left, triton_atten.py:273-274
        qn, kn = logits.shape[-2:]
        logits = logits.masked_fill(torch.arange(kn)[None, :] > torch.arange(qn)[:, None], -math.inf)
    big = float(logits[logits.isfinite()].abs().max())
    m = logits.amax(-1, keepdim=True)
    p = torch.exp2(logits - torch.where(m.isinf(), torch.zeros_like(m), m))
    l = p.sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1 / l, torch.zeros_like(l))  # a row with no visible key is 0
    return (p @ v) * inv, (p @ v.abs()) * inv, v.abs().sum(2, keepdim=True) * inv, big


@functools.lru_cache(maxsize=None)
def case_inputs(d, tag, qn, kn, form):
    gen = torch.Generator().manual_seed(1234)
    qh, kh, dt = (4 if form == "gqa" else 2), 2, DT[tag]
    smooth = form != "no_smooth"
    q = off_ties(torch.randn((1, qh, qn, d), generator=gen).to(dt), False, gen)
    k = off_ties(torch.randn((1, kh, kn, d), generator=gen).to(dt), smooth, gen)
    v = torch.randn((1, kh, kn, d), generator=gen).to(dt)
    mask = None
    if form == "bool":
        mask = torch.rand((1, 1, qn, kn), generator=gen) < 0.7
        mask[..., 5, :] = False  # one row with no visible key
    elif form == "float":
        mask = torch.randn((1, qh, qn, kn), generator=gen).masked_fill(torch.rand((1, qh, qn, kn), generator=gen) < 0.2, -math.inf)
        mask[..., 0] = 0.0
    kw = dict(is_causal=form == "causal", smooth_k=smooth)
    if form == "scale":
        kw.update(scale=0.11, out_dtype=torch.float32)
    sm_scale = kw.get("scale", d ** -0.5)
    return q, k, v, mask, kw, restate(q, k, v, mask, kw["is_causal"], sm_scale, smooth)


@pytest.mark.gpu
@pytest.mark.parametrize("d,tag,qn,kn,form", CASES, ids=lambda c: str(c))
def test_wide_attention_within_its_own_roundings_of_the_float64_restatement(d, tag, qn, kn, form, gpu_device):
    q, k, v, mask, kw, (ref, a, vsum, big) = case_inputs(d, tag, qn, kn, form)
    qd = q.to(gpu_device)
    if form == "token_major":  # memory [Z, N, H, D]: the output takes the query's layout
        qd = q.transpose(1, 2).contiguous().to(gpu_device).transpose(1, 2)
    got = sdnq_hip_atten(qd, k.to(gpu_device), v.to(gpu_device), attn_mask=None if mask is None else mask.to(gpu_device), enable_gqa=form == "gqa", **kw)
    assert got.shape == ref.shape and got.dtype == kw.get("out_dtype", DT[tag])
    if form == "token_major":
        assert got.transpose(1, 2).is_contiguous()
    u = 2.0 ** -8 if tag == "bf16" else 2.0 ** -11
    bound = (u + (2 * kn + 16 * big + 16) * 2.0 ** -24) * (a + ref.abs()) + (2.0 ** -25 * vsum if tag == "f16" else 0)
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\nwide attention DP {(d + 31) // 32 * 32} {tag} {form} q{qn} k{kn}: worst error / bound = {ratio:.3f}, largest |logit| {big:.1f}")
    assert torch.isfinite(got).all() and bool((err <= bound).all()), f"worst error / bound = {ratio:.3f} at {int((err / bound.clamp_min(1e-300)).argmax())}"
    if form == "bool":
        assert not got[..., 5, :].any()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("d", [160, 192, 224, 256])
def test_planted_key_returns_its_value_row_bit_for_bit(d, tag, gpu_device):
    qn, kn, dt = 33, 70, DT[tag]
    planted = torch.tensor([0, kn - 1, 31, 32])  # first key, last key, both sides of a 32-key block edge; query i plants key planted[i % 4]
    gen = torch.Generator().manual_seed(d)
    q = torch.randint(-3, 4, (1, 2, qn, d), generator=gen).float()
    k = torch.randint(-3, 4, (1, 2, kn, d), generator=gen).float()
    q[..., :4] = 0.0
    q[..., torch.arange(qn), torch.arange(qn) % 4] = 127.0  # channel a of the query picks planted key a
    k[..., :4] = -127.0
    k[..., planted, torch.arange(4)] = 127.0                # scores: +-16129 on the picked channel, at most 9 (d - 4) from the rest
    bits = ((0x1000 if tag == "bf16" else 0x0400) + torch.arange(kn * d).view(kn, d)).to(torch.int16)  # positive normal numbers, all distinct
    v = bits.view(dt).expand(1, 2, kn, d).contiguous()
    got = sdnq_hip_atten(q.to(dt).to(gpu_device), k.to(dt).to(gpu_device), v.to(gpu_device), smooth_k=False).cpu()
    want = v[:, :, planted[torch.arange(qn) % 4]]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ"


def test_what_the_host_refuses_for_wide_heads():
    def call(d, **kw):
        x = torch.zeros((1, 2, 8, d), dtype=torch.bfloat16)
        return sdnq_hip_atten(x, x, x, **kw)
    for d in (264, 132):
        with pytest.raises(NotImplementedError, match="head_dim"):
            call(d)
    for kw, name in ((dict(use_hadamard=True), "use_hadamard"), (dict(matmul_dtype="fp8"), "matmul_dtype='fp8'"), (dict(pv_matmul_dtype="int8"), "pv_matmul_dtype='int8'")):
        with pytest.raises(NotImplementedError, match=name):
            call(160, **kw)
    with pytest.raises(_lib.SdnqHipError):
        call(160)
