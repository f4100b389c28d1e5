"""Quantized attention backward for head dims 136 .. 256 (sdnq_amd/csrc/attention_wide_bwd.hip behind sdnq_hip_atten_with_backward).

1. Zero extension: the wide kernels on d = 128 operands padded with zero channels give the narrow kernels' bits (they keep the order of
   every floating-point sum), and zeros above channel 128.
2. Channel roll: rolling the channels of q and k by 64 leaves Out and dv as they are and rolls dq and dk (the scores are integer sums,
   every other sum is per channel).  With 1. this ties every channel tile to the narrow kernels' arithmetic.
3. dV in closed form: k = 0 makes P = 2^-5 for each of 32 keys; small-integer dO makes every sum exact.
4. Random sweep against the CPU restatement (tests/attn_bwd_util.py) on the kernels' own operands, bound 2e-2 as for the narrow kernels
   (tests/test_attention_backward_gpu.py); forward bits, determinism, needs_input_grad subsets, token-major dq, dead mask rows.
5. What the host and the two entry points refuse (no GPU)."""
import ctypes
import math

import pytest
import torch

from sdnq_amd import _lib
from sdnq_amd import attention as A
from tests import attn_bwd_util as R
from tests.test_attention_backward_host import rel

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def bits(x):
    return x.contiguous().view(torch.int16)


def zext(x, d):
    return torch.nn.functional.pad(x, (0, d - x.shape[-1]))


def run(q, k, v, do, mask, kw, need=(True, True, True)):
    q, k, v = (x.detach().requires_grad_(n) for x, n in zip((q, k, v), need))
    out = A.sdnq_hip_atten_with_backward(q, k, v, attn_mask=mask, **kw)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad


def rand(gen, dt, dev, *shape):
    return torch.randn(shape, generator=gen).to(dt).to(dev)


# causal with qn < kn never reaches the key tail; qn >= kn meets the diagonal and the tail in one block
@pytest.mark.gpu
@pytest.mark.parametrize("qn,kn,causal", [(72, 97, False), (72, 97, True), (129, 97, True)])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_zero_extended_operands_give_the_narrow_kernels_bits(tag, qn, kn, causal, gpu_device):
    gen, dt, scale = torch.Generator().manual_seed(3), DT[tag], 0.09
    q, do = rand(gen, dt, gpu_device, 1, 4, qn, 128), rand(gen, dt, gpu_device, 1, 4, qn, 128)
    k, v = rand(gen, dt, gpu_device, 1, 2, kn, 128), rand(gen, dt, gpu_device, 1, 2, kn, 128)
    qq, qs, kq, ks, vt = A.quantize_attn(q, k, v, smooth_k=False)
    out = A.atten_fwd(qq, qs, kq, ks, vt, kn, scale, causal, dt, head_dim=128)
    lse = A.atten_lse(qq, qs, kq, ks, kn, scale, causal, dt, head_dim=128)
    ref = A.atten_bwd(do, out, lse, qq, qs, kq, ks, v, scale, causal)
    for d in (160, 256):
        ws, wqq, wqs, wkq, wks = A.quantize_attn_wide(zext(q, d), zext(k, d), zext(v, d), smooth_k=False)
        wkc = A.unpack_k_fragments(wkq)
        assert torch.equal(wqq[..., :128], qq) and not wqq[..., 128:].any() and torch.equal(wqs, qs)
        assert torch.equal(wkc[..., :128], A.unpack_k_fragments(kq)) and not wkc[..., 128:].any() and torch.equal(wks, ks)
        assert torch.equal(bits(A.atten_wide_lse(ws, 1, 4, 2, qn, kn, d, scale, causal, dt)), bits(lse))
        got = A.atten_wide_bwd(zext(do, d), zext(out, d), lse, ws, zext(v, d), scale, causal)
        for name, a, b in zip(("dq", "dk", "dv"), got, ref):
            assert torch.equal(bits(a[..., :128]), bits(b)), (name, d, int((bits(a[..., :128]) != bits(b)).sum()))
            assert not a[..., 128:].any(), (name, d)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("d", [160, 256])
def test_rolling_the_channels_of_q_and_k_rolls_dq_and_dk(d, tag, gpu_device):
    gen, dt = torch.Generator().manual_seed(d), DT[tag]
    q, do = rand(gen, dt, gpu_device, 1, 2, 40, d), rand(gen, dt, gpu_device, 1, 2, 40, d)
    k, v = rand(gen, dt, gpu_device, 1, 1, 70, d), rand(gen, dt, gpu_device, 1, 1, 70, d)
    out, dq, dk, dv = run(q, k, v, do, None, {})
    out_r, dq_r, dk_r, dv_r = run(q.roll(64, -1), k.roll(64, -1), v, do, None, {})
    assert torch.equal(bits(out_r), bits(out)) and torch.equal(bits(dv_r), bits(dv))
    assert torch.equal(bits(dq_r), bits(dq.roll(64, -1))) and torch.equal(bits(dk_r), bits(dk.roll(64, -1)))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("d", [136, 200, 256])
def test_dv_closed_form_with_uniform_probabilities(d, tag, gpu_device):
    """k = 0: every score is 0, lse = 5, P = 2^-5 exactly.  v is the same small-integer row for every key, so out = v, dP = delta exactly,
    dS = 0 and with it dq and dk; dv = 2^-5 * sum over the 33 queries of both heads of dO, at most 132 / 32 in magnitude: exact in bf16 / f16."""
    gen, dt, qn, kn = torch.Generator().manual_seed(d), DT[tag], 33, 32
    q = rand(gen, dt, gpu_device, 1, 2, qn, d)
    k = torch.zeros((1, 1, kn, d), dtype=dt, device=gpu_device)
    v = (torch.arange(d) % 5 - 2.0).to(dt).expand(1, 1, kn, d).contiguous().to(gpu_device)
    idx = torch.arange(2 * qn).view(1, 2, qn, 1) * 3 + torch.arange(d) * 7
    do = (idx % 5 - 2.0).to(dt).to(gpu_device)  # differs per (head, query, channel), |value| <= 2
    out, dq, dk, dv = run(q, k, v, do, None, {})
    assert torch.equal(out, v[:, :, :1].expand(1, 2, qn, d))
    want = (do.double().sum((1, 2)) * 2.0 ** -5).to(dt).view(1, 1, 1, d).expand(1, 1, kn, d)
    assert torch.equal(dv, want), int((dv != want).sum())
    assert not dq.any() and not dk.any()


# (head dim, dtype, form, smooth_k): every padded head dim in both dtypes; 129 queries on 97 keys (a key tail, 5 query blocks), 4 query heads
# on one KV head throughout
SWEEP = [(136, "bf16", "causal", True), (136, "f16", "bool", False), (160, "bf16", "float", False), (160, "f16", "plain", True),
         (200, "bf16", "bool", True), (200, "f16", "causal", False), (256, "bf16", "plain", False), (256, "f16", "float", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("d,tag,form,smooth", SWEEP, ids=lambda c: str(c))
def test_random_sweep_against_the_restatement(d, tag, form, smooth, gpu_device):
    gen, dt, qn, kn, qh = torch.Generator().manual_seed(7), DT[tag], 129, 97, 4
    q, do = rand(gen, dt, gpu_device, 1, qh, qn, d), rand(gen, dt, gpu_device, 1, qh, qn, d)
    k, v = (torch.randn((1, 1, kn, d), generator=gen) + 2.0).to(dt).to(gpu_device), rand(gen, dt, gpu_device, 1, 1, kn, d)
    mask = None
    if form == "bool":
        mask = torch.rand((1, qh, qn, kn), generator=gen) < 0.7
        mask[:, :, 5] = False  # a row with no visible key
    elif form == "float":  # broadcast over the heads
        mask = torch.randn((1, 1, qn, kn), generator=gen).masked_fill(torch.rand((1, 1, qn, kn), generator=gen) < 0.2, -math.inf)
        mask[..., 0] = 0.0
    mask = None if mask is None else mask.to(gpu_device)
    kw = dict(is_causal=form == "causal", smooth_k=smooth)
    full = run(q, k, v, do, mask, kw)
    out = full[0]
    assert torch.equal(bits(out), bits(A.sdnq_hip_atten(q, k, v, attn_mask=mask, **kw)))
    # the restatement on the operands the kernels read
    m = None if mask is None else A.prepare_mask(mask, qn, kn)
    ws, qq, qs, kq, ks = A.quantize_attn_wide(q, k, v, smooth_k=smooth)
    lse = A.atten_wide_lse(ws, 1, qh, 1, qn, kn, d, d ** -0.5, kw["is_causal"], dt, m)
    want = R.backward(qq.cpu(), qs.cpu(), A.unpack_k_fragments(kq)[:, :, :kn].cpu(), ks[..., :kn].cpu(), v.cpu(), do.cpu(), out.cpu(), lse.cpu(),
                      d ** -0.5, is_causal=kw["is_causal"], mask=None if m is None else m.cpu())
    for name, mine, r in zip(("dq", "dk", "dv"), full[1:], want):
        print(f"\n{name} d {d} {tag} {form}: relative error {rel(mine.cpu(), r):.2e}")
        assert rel(mine.cpu(), r) < 2e-2, (name, rel(mine.cpu(), r))
    for x, y in zip(full, run(q, k, v, do, mask, kw)):  # a second run repeats every bit
        assert torch.equal(bits(x), bits(y))
    for need in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)]:
        for n, x, y in zip(need, full[1:], run(q, k, v, do, mask, kw, need=need)[1:]):
            assert (y is not None) == n and (not n or torch.equal(bits(x), bits(y))), need
    tm = run(q.transpose(1, 2).contiguous().transpose(1, 2), k, v, do, mask, kw)  # [Z, N, H, D] memory
    assert tm[1].stride(2) > tm[1].stride(1) and all(torch.equal(bits(x), bits(y)) for x, y in zip(full, tm))
    if form == "bool":
        assert not full[1][:, :, 5].any()


def test_what_the_host_and_the_entry_points_refuse():
    x = torch.zeros((1, 2, 8, 160), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="use_hadamard"):
        A.sdnq_hip_atten_with_backward(x, x, x, use_hadamard=True)
    for d in (264, 132):
        x = torch.zeros((1, 2, 8, d), dtype=torch.bfloat16)
        with pytest.raises(NotImplementedError, match="head_dim"):
            A.sdnq_hip_atten_with_backward(x, x, x)
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 256

    def rc(fn, base, **broken):
        return fn(*{**base, **broken}.values())
    shape = dict(batch=1, qh=2, kh=2, qn=8, kn=8, d=160)
    mask = dict(mask=None, mask_dtype=0, ms_b=0, ms_h=0, ms_q=0)
    lse = dict(ws=p, ws_bytes=1 << 15, sm_scale=0.125, causal=0, **mask, lse=p, lse_dtype=1, **shape, stream=None)
    bwd = dict(ws=p, ws_bytes=1 << 15, v=p, vst=None, v_dtype=1, out=p, ost=None, grad=p, gst=None, grad_dtype=1, grad_v=p, gvst=None, lse=p,
               sm_scale=0.125, causal=0, **mask, delta=p, dq=p, dqst=None, dq_ch=160, dk=p, dkst=None, dk_ch=160, dv=p, dvst=None, **shape, stream=None)
    for fn, a in ((lib.sdnq_hip_attn_wide_lse, lse), (lib.sdnq_hip_attn_wide_bwd, bwd)):
        assert rc(fn, a, ws=None) == -1 and rc(fn, a, lse=None) == -1      # NULL pointers
        assert rc(fn, a, qh=3) == -3 and rc(fn, a, kn=0) == -3             # head ratio, no keys
        assert rc(fn, a, d=128) == -5 and rc(fn, a, d=264) == -5 and rc(fn, a, d=164) == -5
        assert rc(fn, a, ws=p + 16) == -4                                  # workspace not 256-byte aligned
        assert rc(fn, a, ws_bytes=2 * 8 * 160 + 2 * 32 * 160) == -3        # a workspace that ends inside the four slices
        assert rc(fn, a, mask=p, mask_dtype=5) == -2
    assert rc(lib.sdnq_hip_attn_wide_bwd, bwd, v=p + 2) == -4 and rc(lib.sdnq_hip_attn_wide_bwd, bwd, delta=None) == -1
    assert rc(lib.sdnq_hip_attn_wide_bwd, bwd, dq_ch=168) == -3 and rc(lib.sdnq_hip_attn_wide_bwd, bwd, v_dtype=0) == -2
