"""Which queries and keys did every gradient element count?  Inputs, references, budgets, the case table and the mutants of
tests/test_attention_backward_census.py, for the four kernels of sdnq_amd/csrc/attention_bwd.hip (lse, delta, dQ, dK / dV).

All operands are planted through sdnq_amd.attention.atten_bwd / atten_lse, which take the codes, scales, value, out, lse and grad directly
(K in fragment order: `pack_k_fragments`, keys padded to 32 with zero codes and a NONZERO scale).  Three input families:

  A, census: Q codes one-hot on channels [0, d/2), K codes one-hot on [d/2, d): every score is exactly 0.  q_scale = k_scale = 1, sm_scale a power
     of two, lse[q] = L(q) a small integer, so P = 2^-L exactly; V = 1, dO one-hot 2^L, so P * dP = 1 on every visible pair.  Then
       dq[q, c] / sm = the visible keys whose code channel is c,       dk[key, c] / sm = the visible queries (whole head group) whose code channel is c,
       dv[key, c]    = the visible queries whose dO channel is c
     (`census_closed_form`, float64, written without tests/attn_bwd_util.py).  The channel says who was counted: the index inside the 32-block
     ("inblock") or the block index and the head inside its group ("block").  Accepted: |got / unit - count| <= 0.25; a dropped or doubled item is 1.
     The "delta" variant plants `out` so that dP - delta = sigma(q) 2^M 2^L with sigma = +-1 varying inside a query block and M in {0, 1} varying with
     (batch, head, query block): every count is then weighted by sigma 2^M of its query (equal |dS| inside a quantization block keeps the codes
     exact), which pins attn_delta_kernel and the row delta is read from.  Padded keys carry k_scale 4096: a tail key let through would take the
     block's quantization scale and the real keys' codes to 0.
  B, planted keys: K codes random int8, Q codes of query q = the K codes of key pos(q), k_scale = 1 / |K codes|, q_scale such that the planted score
     is C in the log2 domain with C chosen per case so that it beats every other visible key by 15 in the natural-log domain (cosine < 1 between
     random code rows).  lse is the true lse rounded to the grad dtype.  Reference: `reference64`, the restatement's arithmetic in float64.
  C, random inputs through the HIP forward (tests/test_attention_backward_gpu.py's SWEEP and the abwd_* fixtures) against tests/attn_bwd_util.backward,
     per element.

Budgets (`budgets`), from the reference's own intermediates: tight = one ulp of the grad dtype at the reference value; loose = tight + one flipped
quantization step in the largest contributing block (dq: max_b s_b max|K code[., c]|, dk: max s max|Q code[., c]|, dv: max_q ulp_v(P[q, key]) |dO[q, c]|).
Where float32 arithmetic itself is visible -- a float32 gradient, or the float64 reference of family B -- both tiers also get
(n_terms + d + 8 + 3 ln2 max|S|) 2^-24 sum|terms|: summation order of the n_terms products and of the d products of dP and delta (|terms| carries
P (|dO|.|V| + |out|.|dO|), so the cancellation in dP - delta is covered), eight roundings along P -> dS -> code scale, and the three roundings of the
score chain, which exp2 turns into ln2 |S| 2^-24 each.  Against the float64 reference the flipped step counts only codes that float32 arithmetic can
move at all (`_can_flip`): a planted row's one dominant code is 127 by construction and its neighbours are 0 by seven orders of magnitude, so "the
largest block's step" would be the whole gradient and the check blind.  Under a Hadamard rotation the pre-rotation budgets are carried through |H| and one ulp of
the rotated value is added.  Conditions: no element outside loose, at most 2 % of a tensor outside tight.

`block_loop` is a parameterised float32 copy of the restatement's block loop (padded keys, clamped tail rows, per-head order) on which the CPU tests
run the mutants of MUTANTS.
"""
from __future__ import annotations

import dataclasses
import functools
import math
import zlib

import numpy as np
import torch

from tests import attn_bwd_util as R

BLOCK = 32
QUARTER = 0.25
PAD_K_SCALE = 4096.0
LOG2E = 1.4426950408889634
SM_SCALE = 0.125
TIGHT_SHARE = 0.02
GAP_NAT = 15.0
TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
_PI = [(n & 0x13) | ((n & 4) << 1) | ((n & 8) >> 1) for n in range(32)]


def pack_k_fragments(codes: torch.Tensor) -> torch.Tensor:
    """K codes [Z,KH,KNp,Dp] in key order (KNp % 32 == 0, Dp in (64, 128)) -> fragment order [Z,KH,KNp/32,Dp/32,64,16], the inverse of
    sdnq_amd.attention.unpack_k_fragments: lane g * 32 + rho holds bytes [32 kk + 16 g, + 16) of key pi(rho)."""
    z, kh, knp, dp = codes.shape
    assert knp % BLOCK == 0 and dp % 32 == 0
    t = codes.reshape(z, kh, knp // BLOCK, BLOCK, dp // 32, 2, 16).permute(0, 1, 2, 4, 5, 3, 6)  # [.., kk, g, key, 16]; row rho takes key pi(rho)
    return t[:, :, :, :, :, _PI].reshape(z, kh, knp // BLOCK, dp // 32, 64, 16).contiguous()


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    tag: str                     # value dtype: "f16" | "bf16"
    gdt: str                     # gradient dtype: the value dtype or "f32"
    z: int
    qh: int
    kh: int
    qn: int
    kn: int
    d: int
    causal: bool = False
    mask: str | None = None      # None | "bool" | "f32" | "bf16" | "f16" (additive 0 / -inf)
    bcast: str = ""              # the mask dimensions of size 1: any of "z", "h", "q"
    layout: str | None = None    # None | "tm" (token-major dq) | "vpitch" (V rows 2 d apart) | "dotm" (token-major dO and out)
    assign: str = "inblock"      # census channel classes: "inblock" | "block"
    group: int = 0               # Hadamard group (the kernels then store the padded head dim): census families only

    @property
    def dp(self):
        return 64 if self.d <= 64 else 128

    @property
    def knp(self):
        return (self.kn + 31) // 32 * 32

    @property
    def ratio(self):
        return self.qh // self.kh

    @property
    def instance(self):
        return f"{self.tag}/{self.dp}"

    @property
    def families(self):
        return ("A",) if self.group else ("A", "B")

    @property
    def id(self):
        s = f"{self.tag}-g{self.gdt}-z{self.z}h{self.qh}_{self.kh}-q{self.qn}k{self.kn}d{self.d}-{self.assign}"
        s += "-causal" if self.causal else ""
        s += f"-{self.mask}{'.' + self.bcast if self.bcast else ''}" if self.mask else ""
        s += f"-{self.layout}" if self.layout else ""
        return s + (f"-had{self.group}" if self.group else "")


def _cases():
    C = Case
    return [
        # plain: every head dim, every q / k length, the four instances, the three gradient dtypes, head ratios 1 / 2 / 4 with z > 1
        C("bf16", "bf16", 2, 4, 2, 72, 97, 40),
        C("f16", "f16", 2, 3, 3, 129, 64, 128, assign="block"),
        C("f16", "f32", 2, 4, 1, 33, 200, 64, assign="block"),
        C("bf16", "f32", 1, 2, 2, 31, 33, 128),
        C("bf16", "bf16", 1, 2, 1, 1, 1, 8),
        C("f16", "f16", 1, 2, 2, 32, 1, 24),
        C("f16", "f16", 2, 2, 1, 1, 200, 72, assign="block"),
        C("bf16", "bf16", 1, 4, 4, 32, 64, 80),
        C("bf16", "bf16", 2, 4, 1, 129, 200, 128, assign="block"),
        C("f16", "f32", 1, 2, 1, 72, 97, 8),
        # causal: q_len below, equal to and above kv_len, each with a key tail
        C("bf16", "bf16", 2, 4, 2, 72, 97, 64, causal=True),
        C("f16", "f32", 1, 2, 1, 33, 33, 128, causal=True),
        C("bf16", "bf16", 1, 4, 1, 129, 97, 24, causal=True, assign="block"),
        C("f16", "f16", 2, 2, 2, 31, 33, 80, causal=True),
        C("f16", "f16", 1, 4, 2, 97, 97, 40, causal=True, assign="block"),
        C("bf16", "f32", 1, 1, 1, 1, 1, 64, causal=True),
        # masks: bool and the three additive dtypes; broadcast over batch, heads, queries; a dead row; a (query block, key block) pair hidden
        C("bf16", "bf16", 2, 4, 2, 72, 97, 40, mask="bool"),
        C("f16", "f32", 2, 2, 1, 33, 64, 64, mask="f32", bcast="z"),
        C("bf16", "bf16", 2, 4, 1, 129, 200, 128, mask="bf16", bcast="h", assign="block"),
        C("f16", "f16", 2, 2, 2, 72, 200, 72, mask="f16", bcast="q"),
        C("f16", "f16", 2, 4, 2, 72, 97, 64, causal=True, mask="bool", bcast="zh", assign="block"),   # the `need` subsets run on this one
        C("bf16", "f32", 2, 2, 1, 32, 33, 24, mask="bool", bcast="hq"),
        C("bf16", "bf16", 1, 2, 2, 129, 97, 80, causal=True, mask="f32"),
        C("f16", "f16", 2, 4, 1, 33, 97, 128, mask="bool", bcast="z", assign="block"),
        # layouts
        C("bf16", "bf16", 2, 4, 2, 72, 97, 40, layout="tm", assign="block"),
        C("f16", "f16", 1, 2, 2, 33, 97, 128, layout="vpitch"),
        C("bf16", "f32", 2, 2, 1, 72, 64, 64, layout="dotm"),
        C("f16", "f32", 2, 4, 2, 129, 200, 72, causal=True, mask="bool", layout="tm"),
        # a rotation: dq and dk stored over the padded head dim and rotated back
        C("f16", "f32", 1, 2, 1, 72, 97, 40, group=32),
        C("bf16", "f32", 2, 2, 2, 33, 64, 80, causal=True, group=32, assign="block"),
    ]


CASES = {c.id: c for c in _cases()}
assert len(CASES) == len(_cases())
NEED_CASE = next(c for c in CASES.values() if c.causal and c.mask and c.ratio > 1 and not c.layout and c.gdt != "f32")
NEED_SUBSETS = [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)]


def _rng(case, salt):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{salt}".encode()))


def kv_head(h, qh, kh):
    return h * kh // qh


# ---- masks and visibility ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mask_bool(case):
    """bool numpy in the mask's own (broadcast) shape: random, row 5 dead (where rows are not broadcast), key block 1 hidden from query block 0 and,
    under a query broadcast, from everybody."""
    if case.mask is None:
        return None
    shape = (1 if "z" in case.bcast else case.z, 1 if "h" in case.bcast else case.qh, 1 if "q" in case.bcast else case.qn, case.kn)
    m = _rng(case, "mask").random(shape) < 0.7
    if case.kn > BLOCK:
        m[:, :, :BLOCK, BLOCK:2 * BLOCK] = False
    if "q" not in case.bcast:
        m[:, :, min(5, case.qn - 1), :] = False
    m[:, -1, -1, 0] = True
    m.setflags(write=False)
    return m


def raw_mask(case):
    """The mask as a caller passes it: torch bool, or additive 0 / -inf in the case's mask dtype."""
    m = _mask_bool(case)
    if m is None:
        return None
    t = torch.from_numpy(m.copy())
    if case.mask == "bool":
        return t
    return torch.where(t, 0.0, float("-inf")).to(TDT[case.mask])


def visibility(case):
    """bool numpy [Z, QH, QN, KN]: key j is visible to query i iff (not causal or j <= i) and the mask lets it."""
    vis = np.ones((case.z, case.qh, case.qn, case.kn), dtype=bool)
    if case.causal:
        vis &= np.arange(case.kn)[None, :] <= np.arange(case.qn)[:, None]
    m = _mask_bool(case)
    if m is not None:
        vis &= m
    return vis


# ---- family A: the census ---------------------------------------------------------------------------------------------------------------------
def _census_maps(case):
    """Integer numpy maps: L [Z,QH,QN], w (the weight of a query: 1, or sigma 2^M in the delta variant: `w_delta`), the code channel of every query
    [QH,QN] and key [KH,KN], the dO channel [QH,QN]."""
    z, h, q = np.meshgrid(np.arange(case.z), np.arange(case.qh), np.arange(case.qn), indexing="ij")
    L = (q + 2 * h + 3 * z) % 4
    sigma = np.where((q + h) % 3 == 0, -1, 1)
    M = (q // BLOCK + h + z) % 2
    hh, qq = np.meshgrid(np.arange(case.qh), np.arange(case.qn), indexing="ij")
    kv, kk = np.meshgrid(np.arange(case.kh), np.arange(case.kn), indexing="ij")
    if case.assign == "inblock":
        qcls, kcls = qq % BLOCK, kk % BLOCK + 3 * kv
    else:
        qcls, kcls = (qq // BLOCK) * case.ratio + hh % case.ratio, kk // BLOCK + 3 * kv
    half = case.d // 2
    return dict(L=L, w_delta=sigma * 2 ** M, qch=qcls % half, kch=half + kcls % (case.d - half), och=(qcls + hh // case.ratio) % case.d)


def _one_hot(ch, width, dtype=np.float64):
    return (ch[..., None] == np.arange(width)).astype(dtype)


@functools.lru_cache(maxsize=8)
def census_inputs(case, variant="count"):
    """Operands of family A as CPU torch tensors (left unchanged by everyone: cached): qq int8 [Z,QH,QN,Dp], qs, kc int8 [Z,KH,KNp,Dp] in key
    order, ks [Z,KH,KNp], v [Z,KH,KN,d], do / out [Z,QH,QN,d] and lse [Z,QH,QN] in the gradient dtype, mask as prepare_mask returns it."""
    from sdnq_amd.attention import prepare_mask
    mp = _census_maps(case)
    gdt, vdt = TDT[case.gdt], TDT[case.tag]
    qq = torch.from_numpy(np.broadcast_to(_one_hot(mp["qch"], case.dp, np.int8), (case.z, case.qh, case.qn, case.dp)).copy())
    kc = torch.zeros(case.z, case.kh, case.knp, case.dp, dtype=torch.int8)
    kc[:, :, :case.kn] = torch.from_numpy(_one_hot(mp["kch"], case.dp, np.int8))
    ks = torch.full((case.z, case.kh, case.knp), PAD_K_SCALE)
    ks[:, :, :case.kn] = 1.0
    pw = torch.from_numpy(2.0 ** mp["L"])
    oh = torch.from_numpy(_one_hot(mp["och"], case.d))
    do = (oh * pw[..., None]).to(gdt)
    out = torch.zeros_like(do)
    if variant == "delta":  # delta = 2^L (1 - w): out = 1 - w on the dO channel
        out = (oh * torch.from_numpy(1.0 - mp["w_delta"])[..., None]).to(gdt)
    m = raw_mask(case)
    return dict(case=case, qq=qq, qs=torch.ones(case.z, case.qh, case.qn), kc=kc, ks=ks, v=torch.ones(case.z, case.kh, case.kn, case.d, dtype=vdt),
                do=do, out=out, lse=torch.from_numpy(mp["L"].astype(np.float64)).to(gdt), sm=SM_SCALE, causal=case.causal, raw_mask=m,
                mask=prepare_mask(m, case.qn, case.kn) if m is not None else None, group=case.group)


def rotate64(x, group):
    h = R.hadamard_matrix(group, torch.float64).numpy()
    return (x.reshape(*x.shape[:-1], -1, group) @ h).reshape(x.shape)


def census_closed_form(case, variant="count", vis=None):
    """float64 numpy: dq / sm, dk / sm, dv as counts ([.., d]), and the visible-key count of every row [Z,QH,QN]."""
    mp = _census_maps(case)
    vis = visibility(case) if vis is None else vis
    w = mp["w_delta"].astype(np.float64) if variant == "delta" else np.ones((case.z, case.qh, case.qn))
    k1, q1, o1 = _one_hot(mp["kch"], case.dp), _one_hot(mp["qch"], case.dp), _one_hot(mp["och"], case.d)
    dq = np.zeros((case.z, case.qh, case.qn, case.dp))
    dk = np.zeros((case.z, case.kh, case.kn, case.dp))
    dv = np.zeros((case.z, case.kh, case.kn, case.d))
    for z in range(case.z):
        for h in range(case.qh):
            kv = kv_head(h, case.qh, case.kh)
            v = vis[z, h].astype(np.float64)
            dq[z, h] = w[z, h][:, None] * (v @ k1[kv])
            dk[z, kv] += v.T @ (w[z, h][:, None] * q1[h])
            dv[z, kv] += v.T @ o1[h]
    if case.group:  # as the host rotates the stored padded head dim back: tests/attn_bwd_util.rotate
        dq, dk = (R.rotate(torch.from_numpy(t), case.group).numpy() for t in (dq, dk))
    return dq[..., :case.d], dk[..., :case.d], dv, vis.sum(-1)


def census_errors(case, got, variant="count", vis=None):
    """Worst |got / unit - count| of (dq, dk, dv); got: torch tensors."""
    ref = census_closed_form(case, variant, vis)[:3]
    return [float(np.abs(g.double().numpy() / unit - r).max()) for g, r, unit in zip(got, ref, (SM_SCALE, SM_SCALE, 1.0))]


def assert_census(case, got, variant, label, vis=None, bound=QUARTER):
    ref = census_closed_form(case, variant, vis)[:3]
    worst = []
    for name, g, r, unit in zip(("dq", "dk", "dv"), got, ref, (SM_SCALE, SM_SCALE, 1.0)):
        err = g.double().numpy() / unit - r
        bad = ~(np.abs(err) <= bound)
        if bad.any():
            w = np.unravel_index(np.nanargmax(np.where(np.isnan(err), np.inf, np.abs(err))), err.shape)
            raise AssertionError(f"{label}: {name} off the census in {int(bad.sum())} elements; worst at batch {w[0]} head {w[1]} row {w[2]} channel {w[3]}: "
                                 f"{err[w]:+.3f} counts (got {g.double().numpy()[w] / unit:.6g}, census {r[w]:.6g})")
        worst.append(float(np.abs(err).max()))
    return worst


# ---- family B: planted keys ---------------------------------------------------------------------------------------------------------------------
def planted_positions(case):
    """pos [QH, QN]: the key of every query.  Causal: the diagonal, and past the last key a walk back from it.  Otherwise consecutive queries take
    consecutive keys, wrapping from KN - 1 to 0 in the middle of the queries and shifted by 5 per head: injective per head where QN <= KN."""
    h, q = np.meshgrid(np.arange(case.qh), np.arange(case.qn), indexing="ij")
    if case.causal:
        return np.where(q < case.kn, q, (case.kn - 1 - (q - case.kn)) % case.kn)
    return (q - case.qn // 2 + 5 * h) % case.kn


@functools.lru_cache(maxsize=8)
def planted_inputs(case):
    from sdnq_amd.attention import prepare_mask
    rng = _rng(case, "B")
    z, qh, kh, qn, kn, d, dp, knp = case.z, case.qh, case.kh, case.qn, case.kn, case.d, case.dp, case.knp
    gdt, vdt = TDT[case.gdt], TDT[case.tag]
    kc = np.zeros((z, kh, knp, dp), dtype=np.int64)
    kc[:, :, :kn, :d] = rng.integers(-127, 128, (z, kh, kn, d))
    kc[:, :, :kn, 0] |= 1                                   # no zero row
    pos = planted_positions(case)
    kvs = np.array([kv_head(h, qh, kh) for h in range(qh)])
    qq = kc[:, kvs[:, None], pos]                           # [Z, QH, QN, Dp]
    norm = np.sqrt((kc[:, :, :kn].astype(np.float64) ** 2).sum(-1))
    unit = kc[:, :, :kn] / norm[..., None]
    vis = visibility(case)
    cos = np.einsum("zhqc,zhkc->zhqk", qq / np.sqrt((qq.astype(np.float64) ** 2).sum(-1, keepdims=True)), unit[:, kvs])
    planted = np.zeros_like(vis)
    np.put_along_axis(planted, np.broadcast_to(pos[None, :, :, None], (z, qh, qn, 1)), True, -1)
    live = (vis & planted).any(-1)                          # rows whose planted key is visible
    other = np.where(vis & ~planted, cos, -1.0).max(-1)
    worst = float(other[live].max()) if live.any() and (vis & ~planted)[live].any() else 0.0
    assert worst < 0.999, (case.id, worst)                  # (two parallel code rows: another seed)
    peak = 1.1 * GAP_NAT * LOG2E / (1.0 - max(worst, 0.0))  # the planted score in the log2 domain
    l2 = float(np.float32(SM_SCALE * LOG2E))
    ks = np.full((z, kh, knp), 1.0, dtype=np.float32)
    ks[:, :, :kn] = (1.0 / norm).astype(np.float32)
    qs = (peak / (np.take_along_axis(norm[:, kvs], np.broadcast_to(pos[None], (z, qh, qn)), -1) * l2)).astype(np.float32)
    s = np.einsum("zhqc,zhkc->zhqk", qq, kc[:, kvs, :kn]).astype(np.float64) * qs[..., None] * ks[:, kvs, None, :kn] * l2
    s = np.where(vis, s, -np.inf)
    mx = s.max(-1)
    lse = np.where(np.isneginf(mx), 0.0, np.where(np.isneginf(mx), 0.0, mx) + np.log2(np.exp2(s - np.where(np.isneginf(mx), 0.0, mx)[..., None]).sum(-1).clip(1e-300)))
    runner_up = np.where(planted, -np.inf, s).max(-1)[live]
    gap = (np.where(planted, s, -np.inf).max(-1)[live] - np.where(np.isneginf(runner_up), -1e30, runner_up)) / LOG2E
    m = raw_mask(case)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    return dict(case=case, qq=t(qq, torch.int8), qs=t(qs, torch.float32), kc=t(kc, torch.int8), ks=t(ks, torch.float32),
                v=t(rng.standard_normal((z, kh, kn, d)), vdt), do=t(rng.standard_normal((z, qh, qn, d)), gdt), out=t(rng.standard_normal((z, qh, qn, d)), gdt),
                lse=t(lse, gdt), sm=SM_SCALE, causal=case.causal, raw_mask=m, mask=prepare_mask(m, qn, kn) if m is not None else None, group=0,
                pos=pos, live=live, min_gap_nat=float(gap.min()) if gap.size else math.inf, peak=peak)


# ---- the float64 reference and the budgets ------------------------------------------------------------------------------------------------------
def _hidden(x, z, h, qrows, kn_cols, hide=None):
    """(hidden bool [Q, K], additive float64 [Q, K]) of head (z, h) for the query rows `qrows` over the first `kn_cols` >= KN key columns: the key
    tail, causal, the mask broadcast by its own shape, and `hide` (bool [Z,QH,QN,KN], extra hidden pairs)."""
    kn = x["v"].shape[2]
    keys = torch.arange(kn_cols)
    hid = (keys >= kn)[None, :].expand(len(qrows), -1).clone()
    add = torch.zeros(len(qrows), kn_cols, dtype=torch.float64)
    if x["causal"]:
        hid |= keys[None, :] > qrows[:, None]
    m = x["mask"]
    if m is not None:
        mm = m[0 if m.shape[0] == 1 else z, 0 if m.shape[1] == 1 else h]
        mm = mm.expand(len(qrows), -1) if mm.shape[0] == 1 else mm[qrows]
        if mm.dtype == torch.int8:
            hid[:, :kn] |= mm == 0
        else:
            add[:, :kn] = mm.double()
    if hide is not None:
        hid[:, :kn] |= hide[z, h][qrows]
    return hid, add


def _q8_64(x, dim):
    s = x.abs().amax(dim=dim, keepdim=True) / 127.0
    s = torch.where(s <= 2e-38, torch.ones_like(s), s)
    return torch.floor(x / s + 0.5), s


def _can_flip(x, ex, codes, s, dim):
    """1.0 where float32 arithmetic can move a code of the block: x / s + 0.5 lies closer to an integer than twice the error of x / s -- the
    element's own (ex, absolute) and, through s, that of the block's largest element scaled by the code."""
    val = x / s + 0.5
    margin = (val - torch.round(val)).abs()
    return (margin < 2.0 * (ex / s + codes.abs() * ex.amax(dim=dim, keepdim=True) / (127.0 * s))).double()


def reference64(x, hide=None):
    """The restatement's arithmetic (tests/attn_bwd_util.backward) in float64 over all keys, on the operands dict of `census_inputs` /
    `planted_inputs` (kc / ks may be padded or not).  Returns the unrounded, unrotated dq / dk [.., Dp], dv [.., d] and what `budgets` needs:
    step_* (one quantization step of the largest contributing block), sstep_* (the same over the codes float32 arithmetic can move: `_can_flip`),
    abs_* (sum |terms|), n_* (terms per element), smax."""
    qq, kc, v = x["qq"], x["kc"], x["v"]
    z, qh, qn, dp = qq.shape
    kh, kn, d = v.shape[1], v.shape[2], v.shape[3]
    gdt, vdt = x["do"].dtype, v.dtype
    l2 = float(np.float32(x["sm"] * LOG2E))
    sm = float(np.float32(x["sm"]))
    r = {k: torch.zeros(z, qh, qn, dp, dtype=torch.float64) for k in ("dq", "step_dq", "sstep_dq", "abs_dq")}
    r.update({k: torch.zeros(z, kh, kn, dp, dtype=torch.float64) for k in ("dk", "step_dk", "sstep_dk", "abs_dk")})
    r.update({k: torch.zeros(z, kh, kn, d, dtype=torch.float64) for k in ("dv", "step_dv", "abs_dv")})
    smax = 0.0
    rows = torch.arange(qn)
    for zi in range(z):
        for h in range(qh):
            kv = kv_head(h, qh, kh)
            Q, K = qq[zi, h].double(), kc[zi, kv, :kn].double()
            qs, ks = x["qs"][zi, h].double(), x["ks"][zi, kv, :kn].double()
            hid, add = _hidden(x, zi, h, rows, kn, hide)
            S = (((Q @ K.T) * qs[:, None]) * ks[None]) * l2 + add
            S = S.masked_fill(hid, float("-inf"))
            fin = S[torch.isfinite(S)]
            smax = max(smax, float(fin.abs().max()) if fin.numel() else 0.0)
            P = torch.exp2(S - x["lse"][zi, h].double()[:, None])
            dov, V = x["do"][zi, h].to(vdt).double(), v[zi, kv].double()
            prod = (x["out"][zi, h] * x["do"][zi, h]).double()  # rounded in the gradient dtype
            dS = (P * (dov @ V.T - prod.sum(-1)[:, None])) * sm
            aS = (P * (dov.abs() @ V.abs().T + prod.abs().sum(-1)[:, None])) * sm
            cst = (d + 8 + 3 * math.log(2) * (float(fin.abs().max()) if fin.numel() else 0.0)) * 2.0 ** -24
            xq, smx = dS * ks[None], torch.zeros(qn, 1, dtype=torch.float64)
            for b in range(0, kn, BLOCK):
                codes, s = _q8_64(xq[:, b:b + BLOCK], -1)
                r["dq"][zi, h] += (codes @ K[b:b + BLOCK]) * s
                smx = torch.maximum(smx, torch.where(xq[:, b:b + BLOCK].abs().amax(-1, keepdim=True) > 0, s, torch.zeros_like(s)))
                fl = _can_flip(xq[:, b:b + BLOCK], cst * (aS * ks[None])[:, b:b + BLOCK], codes, s, -1) * s
                r["sstep_dq"][zi, h] = torch.maximum(r["sstep_dq"][zi, h], (fl[:, :, None] * K[b:b + BLOCK].abs()[None]).amax(1))
            r["step_dq"][zi, h] = smx * K.abs().amax(0)[None]
            r["abs_dq"][zi, h] = (aS * ks[None]) @ K.abs()
            y, smk = dS * qs[:, None], torch.zeros(kn, 1, dtype=torch.float64)
            for b in range(0, qn, BLOCK):
                codes, s = _q8_64(y[b:b + BLOCK], 0)
                r["dk"][zi, kv] += (codes.T @ Q[b:b + BLOCK]) * s.T
                smk = torch.maximum(smk, torch.where(y[b:b + BLOCK].abs().amax(0, keepdim=True) > 0, s, torch.zeros_like(s)).T)
                fl = _can_flip(y[b:b + BLOCK], cst * (aS * qs[:, None])[b:b + BLOCK], codes, s, 0) * s
                r["sstep_dk"][zi, kv] = torch.maximum(r["sstep_dk"][zi, kv], (fl.T[:, :, None] * Q[b:b + BLOCK].abs()[None]).amax(1))
            r["step_dk"][zi, kv] = torch.maximum(r["step_dk"][zi, kv], smk * Q.abs().amax(0)[None])
            r["abs_dk"][zi, kv] += (aS * qs[:, None]).T @ Q.abs()
            pdt = vdt if gdt == torch.float32 else gdt
            r["dv"][zi, kv] += P.to(pdt).double().T @ dov
            up = ulp(P, pdt) * (P > 0)
            r["step_dv"][zi, kv] = torch.maximum(r["step_dv"][zi, kv], (up.T[:, :, None] * dov.abs()[None]).amax(1))
            r["abs_dv"][zi, kv] += P.T @ dov.abs()
    r.update(smax=smax, n_dq=kn, n_dk=qn * (qh // kh), n_dv=qn * (qh // kh), d=d, gdt=gdt, group=x["group"])
    return r


def ulp(x, dtype):
    """One unit in the last place of `dtype` at |x| (float64 tensor): the `_ulp` of tests/test_attention_backward_gpu.py, and for float32 its like."""
    if dtype == torch.float32:
        return torch.exp2(torch.floor(torch.log2(torch.clamp(x.abs().double(), min=2.0 ** -126))) - 23)
    from tests.test_attention_backward_gpu import _ulp
    return _ulp(x, dtype).double()


def _rot_abs(t, group):
    """What a Hadamard rotation (entries +- 1 / sqrt(group)) can make of per-channel error bounds."""
    return (t.unflatten(-1, (-1, group)).sum(-1, keepdim=True) / math.sqrt(group)).expand(*t.shape[:-1], -1, group).flatten(-2)


def finish64(r, name):
    """The reference value of r[name] as the kernels deliver it: rounded to the gradient dtype, rotated back and sliced (float64 tensor)."""
    t = r[name].to(r["gdt"]).double()
    if r["group"] and name != "dv":
        t = torch.from_numpy(rotate64(t.numpy(), r["group"])).to(r["gdt"]).double()
    return t[..., :r["d"]]


def budgets(r, name, ref, arith):
    """(tight, loose) float64 tensors for the tensor `name` at the reference values `ref` [.., d]; `arith`: float32 arithmetic is visible."""
    d, gdt, group = r["d"], r["gdt"], r["group"] if name != "dv" else 0
    a = torch.zeros_like(r[name])
    if arith or gdt == torch.float32:
        a = (r["n_" + name] + d + 8 + 3 * math.log(2) * r["smax"]) * 2.0 ** -24 * r["abs_" + name]
    step = r["sstep_" + name] if arith and name != "dv" else r["step_" + name]
    if group:
        pre = ulp(r[name], gdt) if gdt != torch.float32 else torch.zeros_like(a)
        tight = (_rot_abs(pre + a, group))[..., :d] + ulp(ref, gdt)
        return tight, tight + _rot_abs(step, group)[..., :d]
    tight = ulp(ref, gdt) + a[..., :d]
    return tight, tight + step[..., :d]


def tier_report(got, ref, tight, loose):
    """(share of elements outside tight, worst error as a fraction of the loose budget); got / ref: tensors [.., d]."""
    err = (got.double() - ref.double()).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return float((err > tight).double().mean()), float((err / loose).max())


def assert_tiers(got, ref, tight, loose, label, cap=TIGHT_SHARE):
    share, worst = tier_report(got, ref, tight, loose)
    if not (worst <= 1.0 and share <= cap):
        err = (got.double() - ref.double()).abs() / loose
        w = np.unravel_index(int(torch.nan_to_num(err, nan=float("inf")).argmax()), err.shape)
        raise AssertionError(f"{label}: worst error {worst:.3g} of its loose budget at batch {w[0]} head {w[1]} row {w[2]} channel {w[3]} "
                             f"(got {float(got[w]):.6g}, reference {float(ref[w]):.6g}); {share:.2%} of the elements outside one ulp (cap {cap:.0%})")
    return share, worst


# ---- the parameterised block loop and its mutants ------------------------------------------------------------------------------------------------
MUTANTS = {
    # name: (what, the family that must catch it, a family that is blind to it or None)
    "drop_qblock": ("the last query block dropped for the last head of a group", "A", None),
    "causal_start": ("the causal start block of dK / dV one too late", "A", None),
    "diag_hidden": ("the diagonal hidden under causal", "A", None),
    "tail_keys": ("tail keys let through", "A-delta", "A"),   # (a padded key has V = 0: dS = -P delta sm, zero while delta is)
    "clamped_rows": ("rows past q_len counted through the clamped index", "A", None),
    "mask_batch": ("the mask's batch stride ignored", "A", None),
    "mask_head": ("the mask's head stride ignored", "A", None),
    "delta_row": ("delta taken from the neighbouring row", "A-delta", "A"),
    "swap_keys": ("keys 8-15 and 16-23 of a block swapped in the dS.K contraction only", "B", "A"),
    "kvhead_mod": ("h % kv_heads used as the KV head", "A", None),
}


def block_loop(x, mut=None, perturb=None):
    """(dq, dk, dv) as tests/attn_bwd_util.backward computes them (float32, its _q8 and _fma), but block by block as the kernels walk: keys padded
    to 32 with their own scales, the tail query rows through the clamped index, the heads of a group in order.  `mut`: one of MUTANTS.
    `perturb`: a seed; P is then moved by up to 2 float32 ulp per element and dP accumulated in float64 (what another correct kernel may do)."""
    assert mut is None or mut in MUTANTS
    qq, v = x["qq"], x["v"]
    z, qh, qn, dp = qq.shape
    kh, kn, d = v.shape[1], v.shape[2], v.shape[3]
    knp, nqb = (kn + 31) // 32 * 32, (qn + 31) // 32
    gdt, vdt = x["do"].dtype, v.dtype
    kc, ksc = torch.zeros(z, kh, knp, dp, dtype=torch.int8), torch.ones(z, kh, knp)
    kc[:, :, :x["kc"].shape[2]], ksc[:, :, :x["ks"].shape[2]] = x["kc"], x["ks"]
    vp = torch.zeros(z, kh, knp, d)
    vp[:, :, :kn] = v.float()
    l2, sm = torch.tensor(x["sm"] * LOG2E, dtype=torch.float32), torch.tensor(x["sm"], dtype=torch.float32)
    rows = torch.arange(nqb * BLOCK)
    qc, keys = rows.clamp(max=qn - 1), torch.arange(knp)
    gen = torch.Generator().manual_seed(perturb) if perturb is not None else None
    dq, dk, dv = torch.zeros(z, qh, qn, dp), torch.zeros(z, kh, knp, dp), torch.zeros(z, kh, knp, d)
    xm = dict(x)
    if mut in ("mask_batch", "mask_head") and x["mask"] is not None:
        xm["mask"] = x["mask"][:1] if mut == "mask_batch" else x["mask"][:, :1]
    for zi in range(z):
        for h in range(qh):
            kv = h % kh if mut == "kvhead_mod" else kv_head(h, qh, kh)
            Q, K, qs, ks = qq[zi, h].float()[qc], kc[zi, kv].float(), x["qs"][zi, h][qc], ksc[zi, kv]
            hid, add = _hidden(xm, zi, h, qc, knp)
            if mut == "tail_keys":
                hid[:, kn:] = False
                if x["causal"]:
                    hid[:, kn:] = keys[None, kn:] > qc[:, None]
            if mut == "diag_hidden" and x["causal"]:
                hid |= keys[None, :] >= qc[:, None]
            S = (((Q @ K.T) * qs[:, None]) * ks[None]) * l2 + add.float()
            P = torch.exp2(S.masked_fill(hid, float("-inf")) - x["lse"][zi, h].float()[qc][:, None])
            dov = x["do"][zi, h].to(vdt).float()[qc]
            if gen is not None:
                P = P * (1.0 + torch.randint(-2, 3, P.shape, generator=gen).float() * 2.0 ** -23)
                dP = (dov.double() @ vp[zi, kv].double().T).float()
            else:
                dP = dov @ vp[zi, kv].T
            delta = (x["out"][zi, h] * x["do"][zi, h]).float().sum(-1)
            delta = delta[(qc + 1).clamp(max=qn - 1)] if mut == "delta_row" else delta[qc]
            dS = (P * (dP - delta[:, None])) * sm
            # dQ: one (query, 32-key block) at a time
            xq, acc = (dS * ks[None])[:qn], torch.zeros(qn, dp)
            for b in range(0, knp, BLOCK):
                codes, s = R._q8(xq[:, b:b + BLOCK], -1)
                if mut == "swap_keys":
                    codes = codes[:, list(range(8)) + list(range(16, 24)) + list(range(8, 16)) + list(range(24, 32))]
                acc = R._fma(codes @ K[b:b + BLOCK], s, acc)
            dq[zi, h] = acc
            # dK / dV: one (key, 32-query block) at a time; rows past q_len contribute nothing
            live = (torch.ones_like(rows) if mut == "clamped_rows" else (rows < qn)).float()[:, None]
            y, Pk, Qs, dos = (dS * qs[:, None]) * live, P * live, Q * live, dov * live
            Pr = Pk.to(vdt if gdt == torch.float32 else gdt).float()
            for mb in range(nqb):
                if mut == "drop_qblock" and h % (qh // kh) == qh // kh - 1 and mb == nqb - 1:
                    continue
                sl = slice(mb * BLOCK, (mb + 1) * BLOCK)
                codes, s = R._q8(y[sl], 0)
                pr = Pr[sl]
                if mut == "causal_start" and x["causal"]:
                    keep = (keys // BLOCK < mb).float()[None]
                    codes, pr = codes * keep, pr * keep
                dk[zi, kv] = R._fma(codes.T @ Qs[sl], s.T, dk[zi, kv])
                dv[zi, kv] = dv[zi, kv] + pr.T @ dos[sl]
    dq, dk, dv = dq.to(gdt), dk[:, :, :kn].to(gdt), dv[:, :, :kn].to(gdt)
    if x["group"]:
        dq, dk = R.rotate(dq, x["group"]), R.rotate(dk, x["group"])
    return dq[..., :d], dk[..., :d], dv


def restated(x):
    """tests/attn_bwd_util.backward on an operands dict."""
    kn, qn = x["v"].shape[2], x["qq"].shape[2]
    m = x["mask"]
    if m is not None and m.shape[-2] == 1:
        m = m.expand(-1, -1, qn, kn)
    return R.backward(x["qq"], x["qs"], x["kc"][:, :, :kn], x["ks"][..., :kn], x["v"], x["do"], x["out"], x["lse"], x["sm"], is_causal=x["causal"],
                      mask=m, hadamard_group=x["group"])


def random_operands(z, qh, kh, qn, kn, d, tag, gdt, causal=False, seed=0):
    """Random quantized operands with a consistent out and lse (float64 softmax), for the CPU check of the tiers."""
    g = np.random.default_rng(seed)
    dp, vdt, gd = (64 if d <= 64 else 128), TDT[tag], TDT[gdt]
    qq, kc = np.zeros((z, qh, qn, dp), dtype=np.int64), np.zeros((z, kh, kn, dp), dtype=np.int64)
    qq[..., :d], kc[..., :d] = g.integers(-127, 128, (z, qh, qn, d)), g.integers(-127, 128, (z, kh, kn, d))
    qs = (g.uniform(0.5, 1.5, (z, qh, qn)) * 0.02).astype(np.float32)
    ks = (g.uniform(0.5, 1.5, (z, kh, kn)) * 0.02).astype(np.float32)
    v = torch.from_numpy(g.standard_normal((z, kh, kn, d))).to(vdt)
    sm = d ** -0.5
    kvs = [kv_head(h, qh, kh) for h in range(qh)]
    s = np.einsum("zhqc,zhkc->zhqk", qq, kc[:, kvs]).astype(np.float64) * qs[..., None] * ks[:, kvs, None] * float(np.float32(sm * LOG2E))
    if causal:
        s = np.where(np.arange(kn)[None, :] <= np.arange(qn)[:, None], s, -np.inf)
    mx = s.max(-1, keepdims=True)
    p = np.exp2(s - mx)
    lse = mx[..., 0] + np.log2(p.sum(-1))
    out = (p / p.sum(-1, keepdims=True)) @ v[:, kvs].double().numpy()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    return dict(qq=t(qq, torch.int8), qs=t(qs, torch.float32), kc=t(kc, torch.int8), ks=t(ks, torch.float32), v=v,
                do=t(g.standard_normal((z, qh, qn, d)), gd), out=t(out, gd), lse=t(lse, gd), sm=sm, causal=causal, mask=None, raw_mask=None, group=0)
