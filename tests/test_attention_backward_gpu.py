"""Quantized attention backward on the MI355X (sdnq_amd.attention.sdnq_hip_atten_with_backward): the forward against sdnq_hip_atten, the
lse and gradients against the reference kernels' fixtures (tests/golden/abwd_*), the CPU restatement (tests/attn_bwd_util.py) on the
HIP forward's own saved tensors, determinism, layouts, masks and a small training loop."""
import pytest
import torch

from tests import attn_bwd_util as R
from tests.test_attention_backward_host import abwd_names, load, prepared_mask, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _attn():
    from sdnq_amd import attention
    return attention


def _inputs(meta, t, dtype):
    q, k, v, do = (t[key].to(DEV) for key in ("q", "k", "v", "do"))
    mask = t.get("mask")
    return q, k, v, do.to(dtype), (mask.to(DEV) if mask is not None else None)


def _run(q, k, v, do, mask, kw, need=(True, True, True)):
    A = _attn()
    q, k, v = (x.detach().requires_grad_(n) for x, n in zip((q, k, v), need))
    out = A.sdnq_hip_atten_with_backward(q, k, v, attn_mask=mask, **kw)
    out.backward(do)
    return out, q.grad, k.grad, v.grad


def _saved(q, k, v, mask, kw):
    """The HIP forward's saved tensors, through the module's own helpers (what the backward kernels read)."""
    A = _attn()
    d = q.shape[-1]
    group = 0
    if kw.get("use_hadamard"):
        from sdnq_amd.quant_utils import get_hadamard_group_size
        dp = 64 if d <= 64 else 128
        ok, group = get_hadamard_group_size(dp, min(kw.get("hadamard_group_size", 256), dp))
        group = group if ok else 0
    sm = kw.get("scale") or d ** -0.5
    m = A.prepare_mask(mask, q.shape[2], k.shape[2]) if mask is not None else None
    qq, qs, kq, ks, vt = A.quantize_attn(q, k, v, smooth_k=kw.get("smooth_k", True), hadamard_group=group)
    out = A.atten_fwd(qq, qs, kq, ks, vt, k.shape[2], sm, kw.get("is_causal", False), q.dtype, m, head_dim=d)
    lse = A.atten_lse(qq, qs, kq, ks, k.shape[2], sm, kw.get("is_causal", False), q.dtype, m, head_dim=d)
    kcodes = A.unpack_k_fragments(kq)[:, :, :k.shape[2]]
    return dict(q_q=qq, q_scale=qs, k_q=kcodes, k_scale=ks[..., :k.shape[2]], out=out, lse=lse, sm=sm, group=group, mask=m)


def _restated(q, k, v, do, mask, kw):
    s = _saved(q, k, v, mask, kw)
    cpu = {key: (val.cpu() if torch.is_tensor(val) else val) for key, val in s.items()}
    m = cpu["mask"]
    if m is not None:
        m = m.expand(-1, -1, q.shape[2], k.shape[2]) if m.shape[-2] == 1 else m
    return R.backward(cpu["q_q"].view(torch.int8), cpu["q_scale"], cpu["k_q"].view(torch.int8), cpu["k_scale"], v.cpu(), do.cpu(), cpu["out"],
                      cpu["lse"], cpu["sm"], is_causal=kw.get("is_causal", False), mask=m, hadamard_group=cpu["group"])


def _ulp(x, dtype):
    x = x.abs().to(dtype).float()
    e = torch.floor(torch.log2(torch.clamp(x, min=2.0 ** -14)))
    return torch.exp2(e - (10 if dtype == torch.float16 else 7))


@pytest.mark.parametrize("name", abwd_names())
def test_forward_and_lse_match(name):
    A = _attn()
    meta, t = load(name)
    dtype = torch.bfloat16 if meta["dtype"] == "bf16" else torch.float16
    q, k, v, do, mask = _inputs(meta, t, dtype)
    kw = meta["kwargs"]
    out = A.sdnq_hip_atten_with_backward(q, k, v, attn_mask=mask, **kw)
    ref = A.sdnq_hip_atten(q, k, v, attn_mask=mask, **kw)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))  # bit-identical forward
    s = _saved(q, k, v, mask, kw)
    assert torch.equal(s["out"].view(torch.int16), ref.view(torch.int16))
    lse, lref = s["lse"].float().cpu(), t["lse"].float()
    assert (lse - lref).abs().le(_ulp(lref, dtype) * 1.0001).all(), float((lse - lref).abs().max())


@pytest.mark.parametrize("name", abwd_names())
def test_gradients_against_reference(name):
    meta, t = load(name)
    dtype = torch.bfloat16 if meta["dtype"] == "bf16" else torch.float16
    q, k, v, do, mask = _inputs(meta, t, dtype)
    kw = meta["kwargs"]
    _, dq, dk, dv = _run(q, k, v, do, mask, kw)
    mine = {"dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}
    for key in ("dq", "dk", "dv"):
        assert mine[key].dtype == dtype and mine[key].shape == t[key].shape
        ref_err = rel(t[key], t["exact_" + key])
        assert rel(mine[key], t["exact_" + key]) <= 1.25 * ref_err, (key, rel(mine[key], t["exact_" + key]), ref_err)
        if meta["dtype"] == "f16":
            assert rel(mine[key], t[key]) <= 0.25 * ref_err, (key, rel(mine[key], t[key]), ref_err)
    if meta["dtype"] == "bf16":  # the fixtures' bf16 gradients are unrounded: the restatement on the HIP forward's saved tensors instead
        for key, r in zip(("dq", "dk", "dv"), _restated(q, k, v, do, mask, kw)):
            assert rel(mine[key], r) < 2e-2, (key, rel(mine[key], r))


SWEEP = [
    dict(z=2, qh=4, kh=1, qn=72, kn=200, d=64, dtype=torch.bfloat16, kw={}),
    dict(z=1, qh=3, kh=3, qn=129, kn=97, d=128, dtype=torch.bfloat16, kw=dict(is_causal=True)),
    dict(z=1, qh=2, kh=2, qn=64, kn=300, d=96, dtype=torch.float16, kw=dict(smooth_k=False, scale=0.1)),
    dict(z=1, qh=2, kh=1, qn=50, kn=80, d=64, dtype=torch.bfloat16, kw=dict(use_hadamard=True, hadamard_group_size=32)),
    dict(z=1, qh=2, kh=2, qn=40, kn=33, d=24, dtype=torch.float16, kw={}),
]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: f"{c['dtype']}-{c['qh']}x{c['qn']}x{c['kn']}x{c['d']}")
def test_random_sweep_against_restatement(case):
    g = torch.Generator().manual_seed(7)
    q = torch.randn(case["z"], case["qh"], case["qn"], case["d"], generator=g).to(case["dtype"]).to(DEV)
    k = (torch.randn(case["z"], case["kh"], case["kn"], case["d"], generator=g) + 2.0).to(case["dtype"]).to(DEV)
    v = torch.randn(case["z"], case["kh"], case["kn"], case["d"], generator=g).to(case["dtype"]).to(DEV)
    do = torch.randn(case["z"], case["qh"], case["qn"], case["d"], generator=g).to(case["dtype"]).to(DEV)
    _, dq, dk, dv = _run(q, k, v, do, None, case["kw"])
    for key, mine, r in zip(("dq", "dk", "dv"), (dq, dk, dv), _restated(q, k, v, do, None, case["kw"])):
        assert rel(mine.cpu(), r) < 2e-2, (key, rel(mine.cpu(), r))


def _case(name="f16_d128_gqa"):
    meta, t = load(name)
    return _inputs(meta, t, torch.float16) + (meta["kwargs"],)


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)])
def test_needs_input_grad_subsets(need):
    q, k, v, do, mask, kw = _case()
    _, fq, fk, fv = _run(q, k, v, do, mask, kw)
    _, gq, gk, gv = _run(q, k, v, do, mask, kw, need=need)
    for n, full, part in zip(need, (fq, fk, fv), (gq, gk, gv)):
        assert (part is not None) == n
        if n:
            assert torch.equal(full, part)


def test_repeated_runs_bit_identical():
    q, k, v, do, mask, kw = _case()
    a = _run(q, k, v, do, mask, kw)
    b = _run(q, k, v, do, mask, kw)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


def test_strided_and_token_major_inputs():
    q, k, v, do, mask, kw = _case("f16_d64_tail")
    base = _run(q, k, v, do, mask, kw)
    tm = [x.transpose(1, 2).contiguous().transpose(1, 2) for x in (q, k, v)]  # [Z, N, H, D] memory
    got = _run(*tm, do, mask, kw)
    for x, y in zip(base, got):
        assert torch.equal(x, y)
    assert got[1].stride(2) > got[1].stride(1)  # a token-major query gets a token-major dq
    wide = [torch.cat([x, torch.zeros_like(x)], -1)[..., :x.shape[-1]] for x in (q, k, v)]  # row pitch 2 D
    got = _run(*wide, do.transpose(1, 2).contiguous().transpose(1, 2), mask, kw)
    for x, y in zip(base, got):
        assert torch.equal(x, y)


def test_dead_mask_rows_give_zero_gradients():
    meta, t = load("f16_d64_boolmask")
    q, k, v, do, mask = _inputs(meta, t, torch.float16)
    _, dq, dk, dv = _run(q, k, v, do, mask, meta["kwargs"])
    assert dq[:, :, 3].abs().max() == 0 and dq[:, :, 17].abs().max() == 0
    # a dead row contributes nothing to dk / dv: changing its dO changes nothing
    do2 = do.clone()
    do2[:, :, 3] = 7.0
    _, dq2, dk2, dv2 = _run(q, k, v, do2, mask, meta["kwargs"])
    assert torch.equal(dk, dk2) and torch.equal(dv, dv2)


def test_training_loop_tracks_sdpa():
    """The reference README's SDPA swap, for training, on a small attention block (its length rule relaxed so that 128 tokens take the
    quantized path): the loss falls and tracks the same run on torch SDPA."""
    from functools import wraps

    from sdnq.kernels.triton_atten_backward import sdnq_triton_atten_with_backward as sdnq_triton_atten
    sdpa = torch.nn.functional.scaled_dot_product_attention

    @wraps(sdpa)
    def sdpa_sdnq_atten(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, enable_gqa=False, **kwargs):
        if query.device.type != "cpu" and query.shape[-2] >= 32 and key.shape[-2] >= 32 and query.shape[-3] > 1:
            return sdnq_triton_atten(query=query, key=key, value=value, attn_mask=attn_mask, is_causal=is_causal, scale=scale,
                                     enable_gqa=enable_gqa, matmul_dtype="int8", pv_matmul_dtype="disabled", smooth_k=True,
                                     use_hadamard=False, hadamard_group_size=256, do_quantize=True, use_fp16_accum=False, out_dtype=None)
        return sdpa(query=query, key=key, value=value, attn_mask=attn_mask, dropout_p=dropout_p, is_causal=is_causal, scale=scale, **kwargs)

    class Block(torch.nn.Module):
        def __init__(self, dim=256, heads=4):
            super().__init__()
            self.heads = heads
            self.qkv = torch.nn.Linear(dim, 3 * dim)
            self.proj = torch.nn.Linear(dim, dim)

        def forward(self, x, attn):
            b, n, c = x.shape
            q, k, v = self.qkv(x).view(b, n, 3, self.heads, c // self.heads).permute(2, 0, 3, 1, 4)
            return self.proj(attn(q, k, v).transpose(1, 2).reshape(b, n, c))

    def train(attn):
        torch.manual_seed(0)
        blk, teacher = Block().to(DEV, torch.bfloat16), Block().to(DEV, torch.bfloat16)
        x = torch.randn(2, 128, 256, device=DEV, dtype=torch.bfloat16) * 2
        with torch.no_grad():
            target = teacher(x, sdpa)  # a learnable target: another block's output
        opt = torch.optim.SGD(blk.parameters(), lr=2.0)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(blk(x, attn).float(), target.float())
            loss.backward()
            assert all(p.grad is not None for p in blk.parameters())
            opt.step()
            losses.append(loss.item())
        return losses

    ref = train(sdpa)
    mine = train(sdpa_sdnq_atten)
    assert mine[-1] < 0.8 * mine[0]
    for a, b in zip(mine, ref):
        assert abs(a - b) <= 0.03 * abs(b) + 1e-3, (mine, ref)
