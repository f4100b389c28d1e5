"""A CPU restatement, in torch, of the quantized attention backward's arithmetic (sdnq_amd.attention.sdnq_hip_atten_with_backward; the
reference's sdnq_attn_bwd_dq_kernel / sdnq_attn_bwd_dkv_kernel for int8 Q.K^T and P.V in the value dtype), in 32 x 32 blocks:

  S  = ((Q codes . K codes) * q_scale * k_scale) * log2(e) * sm_scale;  causal / masked / tail keys -> -inf
  P  = exp2(S - lse);  dP = dO . V^T (fp32);  delta = sum(out * dO) (product in the output dtype, sum in fp32)
  dS = P * (dP - delta) * sm_scale
  dq += (q8(dS * k_scale) . K codes) * s     per (query, 32-key block)
  dk += (Q codes^T . q8(dS * q_scale)) * s   per (key, 32-query block), the query heads of a group in order
  dv += dO^T . P (P in the value dtype)
  q8(x): s = max|x| / 127 (1 where <= 2e-38), codes = floor(fma(x, 1 / s, 0.5)).
Under a Hadamard rotation dq and dk are rotated back over the padded head dim and sliced.
"""
import os

import numpy as np
import torch

BLOCK = 32


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _q8(x, dim):
    """x [.., 32 along dim ..] -> (codes float, scale) with the block reduced along `dim`."""
    s = x.abs().amax(dim=dim, keepdim=True) * torch.tensor(1.0 / 127.0, dtype=torch.float32)
    s = torch.where(s <= 2e-38, torch.ones_like(s), s)
    inv = torch.tensor(1.0, dtype=torch.float32) / s
    return torch.floor(_fma(x, inv, torch.tensor(0.5))), s


def hadamard_matrix(n, dtype):
    """The reference's (normalised) Hadamard matrices, as stored in tests/golden/hadamard.npz."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hadamard.npz"))
    return torch.from_numpy(z[f"H{n}"].astype(np.float32)).to(dtype)


def rotate(x, group):
    h = hadamard_matrix(group, torch.float32)
    return (x.float().unflatten(-1, (-1, group)) @ h).flatten(-2).to(x.dtype)


def scores(q_q, q_scale, k_q, k_scale, sm_scale, is_causal, mask, lse):
    """P [Z,QH,QN,KN] of the backward (fp32).  k_q / k_scale already expanded to the query heads."""
    s = q_q.float() @ k_q.float().transpose(-1, -2)  # integers below 2^24: exact
    s = ((s * q_scale[..., None]) * k_scale[..., None, :]) * torch.tensor(sm_scale * 1.4426950408889634, dtype=torch.float32)
    qn, kn = s.shape[-2:]
    if is_causal:
        s = s.masked_fill(torch.ones(qn, kn, dtype=torch.bool).triu(1), float("-inf"))
    if mask is not None:
        m = mask
        if m.dtype in (torch.bool, torch.int8):
            s = s.masked_fill(m == 0, float("-inf"))
        else:
            s = s + m.float()
    return torch.exp2(s - lse.float()[..., None])


def backward(q_q, q_scale, k_q, k_scale, v, do, out, lse, sm_scale, is_causal=False, mask=None, hadamard_group=0):
    """(dq, dk, dv) in do.dtype.  q_q [Z,QH,QN,Dp] int8, k_q [Z,KH,KN,Dp] int8 in key order, v [Z,KH,KN,D], do / out [Z,QH,QN,D]."""
    z, qh, qn, dp = q_q.shape
    kh, kn, d = v.shape[1], v.shape[2], v.shape[3]
    rep = qh // kh
    gdt = do.dtype
    kq_e, ks_e, v_e = (t.repeat_interleave(rep, 1) for t in (k_q, k_scale, v))
    p = scores(q_q, q_scale, kq_e, ks_e, sm_scale, is_causal, mask, lse)
    dpm = do.to(v.dtype).float() @ v_e.float().transpose(-1, -2)
    delta = (out * do).float().sum(-1)
    ds = (p * (dpm - delta[..., None])) * torch.tensor(sm_scale, dtype=torch.float32)
    nkb, nqb = -(-kn // BLOCK), -(-qn // BLOCK)
    # dq: blocks of 32 keys
    dq = torch.zeros(z, qh, qn, dp)
    x = ds * ks_e[..., None, :]
    for b in range(nkb):
        sl = slice(b * BLOCK, min(kn, (b + 1) * BLOCK))
        codes, s = _q8(x[..., sl], -1)
        dq = _fma(codes @ kq_e[..., sl, :].float(), s, dq)
    # dk / dv: blocks of 32 queries, the heads of a group in order
    dk = torch.zeros(z, kh, kn, dp)
    dv = torch.zeros(z, kh, kn, d)
    y = ds * q_scale[..., None]
    p_r = p.to(gdt if gdt != torch.float32 else v.dtype).float()
    do_v = do.to(v.dtype).float()
    for i in range(rep):
        hs = [kv * rep + i for kv in range(kh)]
        for b in range(nqb):
            sl = slice(b * BLOCK, min(qn, (b + 1) * BLOCK))
            codes, s = _q8(y[:, hs, sl, :], -2)
            dk = _fma(codes.transpose(-1, -2) @ q_q[:, hs, sl, :].float(), s.transpose(-1, -2), dk)
            dv = dv + p_r[:, hs, sl, :].transpose(-1, -2) @ do_v[:, hs, sl, :]
    dq, dk, dv = dq.to(gdt), dk.to(gdt), dv.to(gdt)
    if hadamard_group:
        dq, dk = rotate(dq, hadamard_group), rotate(dk, hadamard_group)
    return dq[..., :d], dk[..., :d], dv
