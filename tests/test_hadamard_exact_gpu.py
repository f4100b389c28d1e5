"""Every kernel that applies a Hadamard rotation, bit for bit against an expectation no float addition takes part in (tests/hadamard_exact.py):
the rows are integers times one power of two per row, so every partial sum of every butterfly order and of the matrix-core products is exact
and the rotated value is round_T(fl32(S * c)) whatever the order.  Codes, scales, zero points and row sums are the oracle's quantizers applied
to that expected rotation.  A mismatch here is a wrong lane permutation, sign, operand layout, rounding place or dispatch -- never rounding noise.

Shapes are the smallest that reach each kernel form; the derivation from the dispatcher stands beside each table (tests/hadamard_exact.py)
and `rowquant_form` is asserted for every launch."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import hadamard_exact as H

pytestmark = pytest.mark.gpu

from sdnq_amd import _lib, ops  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
MM = {"int8": ops.MM_I8, "fp8": ops.MM_FP8}


def on_device(x32: np.ndarray, tag: str, device) -> torch.Tensor:
    return torch.from_numpy(np.array(x32, dtype=np.float32, order="C")).to(DT[tag]).to(device)  # (a copy: the cached rows are read-only)


def f32_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().contiguous().numpy().view(np.uint32)


def code_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().cpu().view(torch.uint8).numpy()


def assert_same(got: torch.Tensor, want: np.ndarray, what):
    g, w = f32_bits(got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, "mismatches", len(bad), "first at", tuple(int(v) for v in bad[0]),
                           float(g.view(np.float32)[tuple(bad[0])]), float(w.view(np.float32)[tuple(bad[0])]))


@functools.lru_cache(maxsize=8)
def rows_and_rotation(m, k, tag, g):
    x = H.exact_rows(m, k, tag, 7, None, g)
    want = H.expected_rotation(x, g, tag)
    want.setflags(write=False)
    return x, want


# ------------------------------------------------------------------------------------------------
# (a) sdnq_hip_hadamard: hadamard_kernel (wave_hadamard) and hadamard256_kernel (had256_group)
# ------------------------------------------------------------------------------------------------
def hadamard_into(x: torch.Tensor, g: int, y: torch.Tensor):
    rows, k = x.shape
    ops.check(_lib.load().sdnq_hip_hadamard(x.data_ptr(), ops.float_code(x.dtype), rows, k, x.stride(0), g, y.data_ptr(), y.stride(0),
                                            ops._stream(x)), "hadamard")


def ragged_k(g: int):
    """A K that is no multiple of the 512 columns of a wave pass: 520 for groups 4 and 8 (one lane of a second pass), 512 + g up to 128,
    768 for 256; none exists for group 512."""
    return {4: 520, 8: 520, 16: 528, 32: 544, 64: 576, 128: 640, 256: 768}.get(g)


@pytest.mark.parametrize("tag", H.TAGS)
@pytest.mark.parametrize("g", H.GROUPS)
def test_hadamard_exact(g, tag, gpu_device):
    H.require_default_tuning()
    for rows in (1, 5):  # 5: the second workgroup (4 rows each) holds one row, three waves leave at once
        for k in [k for k in (max(g, 8), 3 * max(g, 8), ragged_k(g)) if k]:  # (K is a multiple of 8: one or three lanes at group 4)
            x, want = rows_and_rotation(rows, k, tag, g)
            xd = on_device(x, tag, gpu_device)
            assert_same(ops.hadamard(xd, g), want, (g, tag, rows, k, "contiguous"))
            # ldx / ldy > K, a canary behind every output row (16-byte row pitch: 8 columns)
            wide_x = torch.full((rows, k + 8), 3.0, dtype=DT[tag], device=gpu_device)
            wide_x[:, :k] = xd
            wide_y = torch.full((rows, k + 16), -7.0, dtype=DT[tag], device=gpu_device)
            hadamard_into(wide_x[:, :k], g, wide_y[:, :k])
            assert_same(wide_y[:, :k], want, (g, tag, rows, k, "strided"))
            assert bool((wide_y[:, k:] == -7.0).all()) and bool((wide_x[:, k:] == 3.0).all()), (g, tag, rows, k, "canary")
            # in place, as sdnq_hip_dequant calls it
            inplace = xd.clone()
            hadamard_into(inplace, g, inplace)
            assert_same(inplace, want, (g, tag, rows, k, "in place"))


@pytest.mark.parametrize("tag", H.TAGS)
@pytest.mark.parametrize("g", H.GROUPS)
def test_hadamard_one_hot_census(g, tag, gpu_device):
    """rows = g, row r holds one integer at column r of the row's LAST group (K = 2 g, a multiple of 8): the output is that integer times row
    r of the sign matrix times c -- all g * g signs of the kernel's rotation, and zeros in the other group."""
    H.require_default_tuning()
    k = max(2 * g, 8)
    x = H.one_hot_rows(g, tag, k)
    want = H.expected_rotation(x, g, tag)
    got = ops.hadamard(on_device(x, tag, gpu_device), g)
    v = x[np.arange(g), k - g + np.arange(g)]
    signs = np.sign(got.float().cpu().numpy())
    assert np.array_equal(signs[:, k - g:], np.sign(v)[:, None] * H.sign_matrix(g)), (g, tag, "signs")
    assert_same(got, want, (g, tag, "one-hot"))


# ------------------------------------------------------------------------------------------------
# (b), (c): the fused rotate + quantize kernels
# ------------------------------------------------------------------------------------------------
def check_quantized(xd, want_rot, tag, g, mode, what, want_xrot=True, prefetch=None, lp=False):
    """One launch of the row quantizer in `mode` ("int8": symmetric + row sums, "fp8", "asym") against the oracle's quantizer on the expected
    rotation (g = 0: on the rows themselves)."""
    rs_want = zp_want = None
    if lp and mode == "asym":
        xq, xs, xzp, rs, xrot = ops.rowquant_lp_asym(xd, g, want_rowsum=True, want_xrot=want_xrot)
        q, s, zp_want = O.rowquant_asym_lp(want_rot, tag)
        rs_want = q.astype(np.int32).sum(-1)
    elif lp:
        xq, xs, rs, xrot = ops.rowquant_lp(xd, MM[mode], g, want_rowsum=(mode == "int8"), want_xrot=want_xrot)
        xzp = None
        q, s, rs_want = O.rowquant_lp(want_rot, mode, tag)
    elif mode == "asym":
        xq, xs, rs, xrot, xzp = ops.rowquant(xd, ops.MM_I8, g, want_rowsum=True, want_xrot=want_xrot, prefetch=prefetch, asymmetric=True)
        q, s, zp_want = O.rowquant_asym(want_rot)
        rs_want = q.astype(np.int32).sum(-1)
    else:
        xq, xs, rs, xrot = ops.rowquant(xd, MM[mode], g, want_rowsum=(mode == "int8"), want_xrot=want_xrot, prefetch=prefetch)
        xzp = None
        q, s, rs_want = O.rowquant(want_rot, mode)
    if g and want_xrot:
        assert_same(xrot, want_rot, (what, "rotated copy"))
    else:
        assert xrot is None
    assert_same(xs.reshape(-1), s, (what, "scales"))
    bad = np.argwhere(code_bits(xq) != q.view(np.uint8))
    assert bad.size == 0, (what, "codes", len(bad), "first at", tuple(int(v) for v in bad[0]))
    if zp_want is not None:
        assert_same(xzp, zp_want, (what, "zero points"))
    if rs_want is not None:
        assert np.array_equal(rs.cpu().numpy(), rs_want), (what, "row sums")


@pytest.mark.parametrize("form,m,k", H.HAD256_CASES, ids=[f"{f}-m{m}-k{k}" for f, m, k in H.HAD256_CASES])
def test_rowquant_had256_exact(form, m, k, gpu_device):
    for tag in ("bf16", "f16"):
        assert H.rowquant_form(m, k, tag, 256) == form
        x, want = rows_and_rotation(m, k, tag, 256)
        xd = on_device(x, tag, gpu_device)
        for mode in ("int8", "fp8"):
            for want_xrot in (True, False):
                check_quantized(xd, want, tag, 256, mode, (form, m, k, tag, mode, want_xrot), want_xrot=want_xrot)


def prefetch_tensor(device):
    """300000 bytes: 18750 16-byte vectors, ten prefetch workgroups of 2048 vectors, the last one ragged."""
    return torch.arange(300000, device=device, dtype=torch.int32).to(torch.uint8)


_ROWQ_IDS = [f"{f}-m{m}-k{k}{'-prefetch' if pf else ''}" for f, m, k, pf in H.ROWQUANT_CASES]


@pytest.mark.parametrize("form,m,k,pf", H.ROWQUANT_CASES, ids=_ROWQ_IDS)
def test_rowquant_fwht_exact(form, m, k, pf, gpu_device):
    prefetch = prefetch_tensor(gpu_device) if pf else None
    for tag, g, mode in H.fwht_configs(m, k, pf):
        assert H.rowquant_form(m, k, tag, g, mode == "asym", False, pf) == "fwht-" + form
        x, want = rows_and_rotation(m, k, tag, g)
        check_quantized(on_device(x, tag, gpu_device), want, tag, g, mode, (form, m, k, tag, g, mode), prefetch=prefetch)


@pytest.mark.parametrize("form,m,k", H.LP_CASES, ids=[f"{f}-m{m}-k{k}" for f, m, k in H.LP_CASES])
def test_rowquant_lp_rotated_exact(form, m, k, gpu_device):
    for tag in ("bf16", "f16"):
        for g in (256, 128 if k % 512 else 512):
            x, want = rows_and_rotation(m, k, tag, g)
            xd = on_device(x, tag, gpu_device)
            for mode in ("int8", "fp8", "asym"):
                assert H.rowquant_form(m, k, tag, g, mode == "asym", True) == "fwht-" + form
                check_quantized(xd, want, tag, g, mode, (form, m, k, tag, g, mode), lp=True)


# ------------------------------------------------------------------------------------------------
# (d) the same table without a rotation, on the Gaussian rows of test_gpu_parity.py::test_rowquant_bit_exact_vs_oracle, whose six shapes
#     select plain NP2 / NP3 one-wave, W4 NP3 and W4 NP8 only
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,m,k,pf", H.ROWQUANT_CASES, ids=_ROWQ_IDS)
def test_rowquant_plain_forms_vs_oracle(form, m, k, pf, gpu_device):
    prefetch = prefetch_tensor(gpu_device) if pf else None
    gen = torch.Generator().manual_seed(k + m)
    x = torch.randn(m, k, generator=gen) * 3
    x[:, 5 % k] *= 20
    x[min(3, m - 1)] = 0
    for tag in H.TAGS:
        assert H.rowquant_form(m, k, tag, 0, False, False, pf) == "plain-" + form
        xt = x.to(DT[tag])
        xf = xt.float().numpy()
        for mode in ("int8", "fp8", "asym"):
            check_quantized(xt.to(gpu_device), xf, tag, 0, mode, (form, m, k, tag, mode), prefetch=prefetch)


@pytest.mark.parametrize("form,m,k", H.LP_CASES, ids=[f"{f}-m{m}-k{k}" for f, m, k in H.LP_CASES])
def test_rowquant_lp_plain_vs_oracle(form, m, k, gpu_device):
    """The 16-bit quantizers without a rotation at the same two shapes (the table of tests/hadamard_exact.py names this form too)."""
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(k + m)) * 3
    x[:, 5] *= 20
    x[1] = 0
    for tag in ("bf16", "f16"):
        xt = x.to(DT[tag])
        for mode in ("int8", "fp8", "asym"):
            assert H.rowquant_form(m, k, tag, 0, mode == "asym", True) == "plain-" + form
            check_quantized(xt.to(gpu_device), xt.float().numpy(), tag, 0, mode, (form, m, k, tag, mode), lp=True)


# ------------------------------------------------------------------------------------------------
# (f) the weight side: ops.embedding (wave_hadamard16, a lane owns 16 columns) and ops.dequant (sdnq_hip_hadamard in place), all eight groups
# ------------------------------------------------------------------------------------------------
WEIGHT_N, WEIGHT_K = 12, 1536   # 1536 = 3 * 512: every group divides it; the embedding's second 1024-column chunk is half live


@functools.lru_cache(maxsize=None)
def planted_weight(wdt: str):
    """Stored bytes chosen, not quantized: int8 codes with one power-of-two scale per row, or uint4 codes in groups of 16 whose scales are
    2^e or 2^(e+1) of the row's e with the zero point -8 s.  Every dequantized element v s (+ z) is an integer times the row's 2^e, at most
    128 (int8) / 16 (uint4) of them: a number of every dtype, and a row `expected_rotation` takes.
    Returns (stored uint8, scale [N, G] f32, zero point | None, group size, dequantized weight float32 [N, K])."""
    n, k = WEIGHT_N, WEIGHT_K
    rng = H._rng("weight", wdt)
    e = rng.integers(-6, 3, size=(n, 1))
    if wdt == "int8":
        stored = rng.integers(0, 256, size=n * k).astype(np.uint8)
        gs, scale, zp = k, np.exp2(e.astype(np.float64)), None
    else:
        stored = O.pack_codes(rng.integers(0, 16, size=n * k), 4)
        gs = 16
        scale = np.exp2((e + rng.integers(0, 2, size=(n, k // gs))).astype(np.float64))
        zp = -8.0 * scale
    vals = O.weight_values(stored, wdt, (n, k)).astype(np.float64)
    w = vals * np.repeat(scale, gs, axis=1) + (0.0 if zp is None else np.repeat(zp, gs, axis=1))
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)
    for tag in H.TAGS:
        assert np.array_equal(O.round_dtype(w32, tag), w32), (wdt, tag, "a planted weight element is not a number of the dtype")
    H.split_rows(w32)  # integer rows times a power of two: asserted there
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return stored, f(scale), f(zp), gs, w32


def device_weight(wdt: str, device):
    stored, scale, zp, gs, _ = planted_weight(wdt)
    t = lambda a: None if a is None else torch.from_numpy(a.copy()).to(device)  # noqa: E731
    return ops.make_quant_weight(wdt, t(stored), t(scale), t(zp), None, None, WEIGHT_N, WEIGHT_K, gs, transposed=False)


@pytest.mark.parametrize("wdt", ["int8", "uint4"])
@pytest.mark.parametrize("g", H.GROUPS)
def test_weight_side_rotation_exact(g, wdt, gpu_device):
    w = planted_weight(wdt)[4]
    qw = device_weight(wdt, gpu_device)
    ids = np.array([3, 0, 11, 3, 7], dtype=np.int64)   # 5 ids x 2 chunks = 10 waves: the third workgroup holds two
    for tag in H.TAGS:
        rot = H.expected_rotation(w, g, tag)           # round_T(q s) is q s itself (asserted in planted_weight)
        assert_same(ops.dequant(qw, DT[tag], g), rot, (g, wdt, tag, "dequant"))
        for ids_dt in (torch.int64, torch.int32):
            got = ops.embedding(qw, torch.from_numpy(ids).to(ids_dt).to(gpu_device), DT[tag], g)
            assert_same(got, rot[ids], (g, wdt, tag, ids_dt, "embedding"))
        es = 39.191835884530846  # sqrt(1536): no power of two, the product rounds a second time
        scaled = O.round_dtype((rot[ids] * np.float32(es)).astype(np.float32), tag)
        got = ops.embedding(qw, torch.from_numpy(ids).to(gpu_device), DT[tag], g, embed_scale=es)
        assert_same(got, scaled, (g, wdt, tag, "embedding * embed_scale"))


# ------------------------------------------------------------------------------------------------
# (e) attention prepare under a rotation: attn_quant_block (attention.hip) and its fp8 / quantized-V form (attention_var.hip)
# ------------------------------------------------------------------------------------------------
ATTN_QH, ATTN_KH, ATTN_QN = 4, 2, 37   # GQA 4:2; 37 queries: the last Q workgroup is ragged


def smooth_keys(kh: int, kn: int, d: int, tag: str, seed: int) -> np.ndarray:
    """float32 [1, kh, kn, d] integer tokens whose channel means are integers: |k| <= limit / 2 - 2, then the channel sum's remainder
    mod kn is taken off, one from each of that many tokens.  kn is a power of two: sum / kn is exact as a division and as a product with
    the reciprocal; k - mean is an integer of at most limit - 3, a number of `tag`, and the rotation's sums stay exact."""
    assert kn & (kn - 1) == 0
    lim = H.LIMIT[tag] // 2 - 2
    rng = H._rng("keys", kh, kn, d, tag, seed)
    k = rng.integers(-lim, lim + 1, size=(kh, kn, d))
    k[:, 1] = 0                                          # a token that is all zero before the mean
    rem = k.sum(axis=1) % kn                             # [kh, d], in [0, kn)
    k -= (np.arange(kn)[None, :, None] < rem[:, None, :]).astype(np.int64)
    assert not (k.sum(axis=1) % kn).any() and np.abs(k).max() <= lim + 1
    diff = k - k.sum(axis=1, keepdims=True) // kn
    d32 = diff.astype(np.float32)
    assert np.array_equal(O.round_dtype(d32, tag), d32)
    return k.astype(np.float32)[None]


def attn_inputs(d: int, kn: int, g: int, tag: str, smooth: bool):
    q = H.exact_rows(ATTN_QH * ATTN_QN, d, tag, 11, None, g).reshape(1, ATTN_QH, ATTN_QN, d)
    v = H.exact_rows(ATTN_KH * kn, d, tag, 13, None, g).reshape(1, ATTN_KH, kn, d)
    k = smooth_keys(ATTN_KH, kn, d, tag, 12) if smooth else H.exact_rows(ATTN_KH * kn, d, tag, 12, None, g).reshape(1, ATTN_KH, kn, d)
    return q, k, v


# head dim -> groups: 4, 8, 64 and the head dim; 40 is zero-padded to 64 inside the kernels and takes the groups that divide 40
ATTN_GROUPS = {64: (4, 8, 64), 128: (4, 8, 64, 128), 40: (4, 8)}
# (kv_len, smooth_k): 32 and 160 keys (one key block, five); the mean at 32 keys inside the K workgroups (kv_len <= 256) and at 512 keys from
# the channel-sum workgroups of the launch before
ATTN_KEYS = ((32, False), (160, False), (32, True), (512, True))


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("d", sorted(ATTN_GROUPS))
def test_attention_prepare_rotated_exact(d, tag, gpu_device):
    from sdnq_amd import attention as A
    H.require_default_tuning()
    dp = 64 if d <= 64 else 128
    for g in ATTN_GROUPS[d]:
        for kn, smooth in ATTN_KEYS:
            q, k, v = attn_inputs(d, kn, g, tag, smooth)
            # Q token-major in memory ([Z, N, H, D]), handed over as its [Z, H, N, D] view
            qd = on_device(q.transpose(0, 2, 1, 3), tag, gpu_device).transpose(1, 2)
            assert not qd.is_contiguous()
            kd, vd = on_device(k, tag, gpu_device), on_device(v, tag, gpu_device)
            for mm, pv in (("int8", None), ("fp8", "int8")):
                what = (d, tag, g, kn, smooth, mm, pv)
                with np.errstate(all="ignore"):
                    _, ref = O.attention(q, k, v, tag, smooth_k=smooth, hadamard_group=g, want_intermediates=True, matmul_dtype=mm, pv_matmul_dtype=pv)
                if pv is None:
                    qq, qs, kq, ks, vt = A.quantize_attn(qd, kd, vd, smooth_k=smooth, hadamard_group=g)
                    assert torch.equal(A.unpack_v_fragments(vt)[:, :, :kn, :d], vd), (what, "V in the value dtype")
                else:
                    qq, qs, kq, ks, vt, vs = A.quantize_attn_ex(qd, kd, vd, smooth_k=smooth, hadamard_group=g, matmul_dtype=mm, pv_matmul_dtype=pv)
                    v_rows = A.unpack_v8_fragments(vt)
                    assert np.array_equal(code_bits(v_rows[:, :, :kn, :d]), ref["v_q"].view(np.uint8)), (what, "V codes")
                    assert_same(vs[..., :kn], ref["v_scale"], (what, "V scales"))
                    assert not v_rows[:, :, kn:].any() and not v_rows[..., d:].any() and not vs[..., kn:].any()
                k_rows = A.unpack_k_fragments(kq)
                assert tuple(qq.shape) == (1, ATTN_QH, ATTN_QN, dp) and tuple(k_rows.shape) == (1, ATTN_KH, -(-kn // 32) * 32, dp)
                assert np.array_equal(code_bits(qq[..., :d]), ref["q_q"].view(np.uint8)), (what, "Q codes")
                assert_same(qs, ref["q_scale"], (what, "Q scales"))
                assert np.array_equal(code_bits(k_rows[:, :, :kn, :d]), ref["k_q"].view(np.uint8)), (what, "K codes")
                assert_same(ks[..., :kn], ref["k_scale"], (what, "K scales"))
                assert not qq[..., d:].any() and not k_rows[..., d:].any() and not k_rows[:, :, kn:].any() and not ks[..., kn:].any()
