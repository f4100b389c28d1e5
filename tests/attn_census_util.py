"""Which keys did every query see?  Inputs, references, the case table and the two assertion helpers of tests/test_attention_census.py.

Two input families for the quantized attention forward (sdnq_amd.attention.sdnq_hip_atten), both checked against references computed on the CPU:

  A, key census: Q = 0, so every score is equal and P is exactly 1 on every visible key in every format (f16, bf16, int8, e4m3).  K is random
     (randn + 1: smooth-K and the quantizers run on real data), V[j, c] = 1 if j % D == c else 0.  Then out[q] = (vis[q] @ V) / vis[q].sum():
     channel c of a row counts the visible keys congruent to c, and a key dropped, counted twice or wrongly masked moves its channel by at least
     0.98 / n.  Accepted: |got - ref| * n_visible <= 0.25 (a quarter of ONE key's contribution); the legitimate error is a few float32 ulp.
  B, planted keys: K and V random, query i = 3 K[pos(i)]: about e^15 of the row's mass sits on key pos(i) and out[i] ~ V[pos(i)].  pos walks the
     critical keys (first / last key of every 32-key block, the last valid key, under causal the diagonal).  Exercises the running maximum, the
     rescale and the merge of key parts, and K and V sharing one key order.  Reference: oracle.attention, at the limits of tests/test_attention.py.

`launch_path` restates the launcher's choice among its five paths (sdnq_amd/csrc/attention.hip:828-848) and `key_parts` the share of every key
part (attention.hip:451-474): the case table below is built so that every (path x form) cell is hit, and the CPU tests check that through them.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import zlib

import numpy as np

from oracle import oracle as O

BLOCK = 32
QUARTER_KEY = 0.25

# the launcher's tuning aids (attention.hip:829, 837, 845) and the host's A/B aid that takes the one-launch route away (attention.py, _Q16):
# read once per process, like the library does
TUNING_ENV = ("SDNQ_HIP_ATTN_SPLIT", "SDNQ_HIP_ATTN_SPLIT_TARGET", "SDNQ_HIP_ATTN_SHARED", "SDNQ_HIP_ATTN_Q16")
_TUNING_SET = {k: os.environ[k] for k in TUNING_ENV if k in os.environ}


def require_default_tuning():
    """The case table is laid out for the launcher's own rule: with a tuning override the cases would run on other paths than they claim."""
    assert not _TUNING_SET, f"unset {sorted(_TUNING_SET)}: the attention census needs the launcher's own choice of path, got overrides {_TUNING_SET}"


def launch_path(z, qh, qn, kn, d, causal, masked) -> str:
    """inline | whole | split2 | split4 | shared for the default formats (int8 Q.K^T, P.V in the value dtype), no Hadamard rotation, no tuning
    override: the rule of attn_fwd_impl (attention.hip:828-848) behind sdnq_hip_attn's single launch for at most 128 keys (attention.hip:889-897)."""
    if kn <= 128:                                                  # ATTN_SINGLE_MAX_KEYS: K / V quantized in LDS by the forward launch (raw -> split 1)
        return "inline"
    dp = 64 if d <= 64 else 128                                    # attn_padded_dim
    tiles = z * qh * ((qn + 31) // 32)                             # :830
    want_shared = dp == 128 and kn >= 2048 and not causal and not masked  # :833
    split = 1
    if not want_shared:                                            # :839-842, split_target 4096
        kblocks = (kn + 31) // 32
        while split < 4 and tiles * split < 4096 and kblocks >= 4 * (split * 2):
            split *= 2
    if split > 1:
        return f"split{split}"
    return "shared" if want_shared else "whole"                    # :846 (kn >= 64 holds: kn >= 2048)


def key_parts(kn, q0, split, causal, masked):
    """The key blocks of the query tile starting at row q0, per key part, as attention.hip:451-474 deals them: a list of `split` lists of block
    indices.  Without a mask the plain blocks are divided evenly and the one tail / diagonal block goes to the last part; with a mask all blocks
    are divided evenly."""
    nkb, n_plain = (kn + 31) // 32, kn // 32
    if causal:
        lim = q0 // 32 + 1
        nkb, n_plain = min(nkb, lim), min(n_plain, lim - 1)
    parts = []
    for part in range(split):
        if masked:
            mper = (nkb + split - 1) // split
            mlo = min(part * mper, nkb)
            parts.append(list(range(mlo, min(mlo + mper, nkb))))
        else:
            per = (n_plain + split - 1) // split
            lo = min(part * per, n_plain)
            blocks = list(range(lo, min(lo + per, n_plain)))
            if part == split - 1:
                blocks += list(range(n_plain, nkb))
            parts.append(blocks)
    return parts


def critical_keys(kn):
    """First and last key of every 32-key block and the last valid key."""
    return sorted({b for b in range(0, kn, BLOCK)} | {min(b + BLOCK - 1, kn - 1) for b in range(0, kn, BLOCK)} | {kn - 1})


# ---- the case table --------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    tag: str            # "f16" | "bf16"
    z: int
    qh: int
    kh: int
    qn: int
    kn: int
    d: int
    causal: bool = False
    mask: str | None = None      # None | "bool" | "f32" | "bf16" ([1, 1, QN, KN]) | "bcast" (float32 [QH, 1, KN])
    mm: str = "int8"
    pv: str | None = None

    @property
    def variant(self):
        return self.mm != "int8" or self.pv is not None

    @property
    def form(self):
        return ("mask+causal" if self.causal else "mask") if self.mask else ("causal" if self.causal else "plain")

    @property
    def path(self):
        return "variant" if self.variant else launch_path(self.z, self.qh, self.qn, self.kn, self.d, self.causal, self.mask is not None)

    @property
    def split(self):
        return {"split2": 2, "split4": 4}.get(self.path, 1)

    @property
    def fmt(self):
        return f"{self.mm}/{self.pv or 'value'}"

    @property
    def id(self):
        s = f"{self.path}-{self.tag}-z{self.z}h{self.qh}_{self.kh}-q{self.qn}k{self.kn}d{self.d}-{self.form}"
        if self.mask not in (None, "bool"):
            s += f"-{self.mask}"
        return s + (f"-{self.mm}-{self.pv}" if self.variant else "")

    def kwargs(self):
        kw = dict(is_causal=self.causal)
        if self.variant:
            kw.update(matmul_dtype=self.mm, pv_matmul_dtype=self.pv)
        return kw


# (dtype, batch, query heads, kv heads, head dim), dealt round-robin over the cells of a path: every path meets both dtypes, head dims 64, 128 and a
# padded one, equal and grouped heads (checked by test_case_table_covers_every_path_and_form)
_COMBOS = (("f16", 1, 2, 2, 64), ("bf16", 1, 4, 1, 128), ("f16", 2, 4, 2, 80), ("bf16", 1, 3, 3, 40), ("f16", 1, 4, 1, 128), ("bf16", 2, 2, 2, 64))
_SHARED_COMBOS = (("f16", 1, 4, 1, 128), ("bf16", 1, 2, 2, 128), ("bf16", 1, 4, 2, 128), ("f16", 1, 4, 4, 128))  # the largest: 4 x 130 x 2100 x 128


def _default_cases():
    cells = []  # (qn, kn, causal, mask)
    for kn in (1, 33, 128, 129, 224):                              # inline / whole: plain, causal, mask
        cells += [(70, kn, False, None), (kn, kn, True, None), (100, kn, False, "bool")]
    for kns, below, above in (((225, 256, 300, 480), (70, 300), (600, 300)), ((481, 512, 520, 544, 581), (70, 520), (600, 520))):  # split 2 / split 4
        for kn in kns:
            cells += [(70, kn, False, None), (kn, kn, True, None), (100, kn, False, "bool"), (kn, kn, True, "bool")]
        cells += [(*below, True, None), (*above, True, None), (*below, True, "bool"), (*above, True, "bool")]
        cells += [(100, kns[2], False, "f32"), (100, kns[-1], False, "bf16"), (100, kns[1], False, "bcast")]
    out = [Case(*_COMBOS[i % len(_COMBOS)][:4], qn, kn, _COMBOS[i % len(_COMBOS)][4], causal, mask) for i, (qn, kn, causal, mask) in enumerate(cells)]
    for i, (qn, kn) in enumerate(((33, 2048), (130, 2100), (130, 2048), (33, 2100))):
        out.append(Case(*_SHARED_COMBOS[i][:4], qn, kn, 128))
    return out


VARIANT_FORMATS = (("fp8", None), ("int8", "int8"), ("int8", "fp8"), ("fp8", "fp8"), ("fp8", "int8"), ("int8", "float16"))
VARIANT_KN = (33, 96, 129, 160, 300, 581)  # 2, 3, 5, 5, 10 and 19 key blocks
VARIANT_FORMS = ("plain", "causal", "causal-below", "causal-above", "mask", "mask+causal")


def _variant_cases():
    """A Latin square: format (a + b) % 6 at key length a and form b, so every format meets every key length and every form once; head dim 128 at
    every other key length (so every format runs both), bf16 on the plain column (every format and key length once)."""
    out = []
    for a, kn in enumerate(VARIANT_KN):
        for b, form in enumerate(VARIANT_FORMS):
            mm, pv = VARIANT_FORMATS[(a + b) % 6]
            causal = "causal" in form
            qn = {"causal": kn, "causal-below": kn // 2 + 3, "causal-above": kn + 40, "mask+causal": kn, "mask": 100}.get(form, 70)
            qh, kh = ((2, 2), (2, 1))[b % 2]
            out.append(Case("bf16" if b == 0 else "f16", 1, qh, kh, qn, kn, 128 if a % 2 else 64, causal, "bool" if "mask" in form else None, mm, pv))
    return out


DEFAULT_CASES = _default_cases()
VARIANT_CASES = _variant_cases()
CASES = {c.id: c for c in DEFAULT_CASES + VARIANT_CASES}
assert len(CASES) == len(DEFAULT_CASES) + len(VARIANT_CASES)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _rng(case, salt):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{salt}".encode()))


def build_mask(case):
    """bool [1, 1, QN, KN] (or [QH, 1, KN] for "bcast"): random, row 5 dead, whole 32-key blocks masked -- block 1 for every query, and everything
    key part 1 sees of the last full query tile and key part 0 of the one before it (`key_parts`), so one part of their merge has no visible key
    while the other tiles merge live parts.  "bcast": head h loses all blocks of part h % split."""
    if case.mask is None:
        return None
    rng, kn, qn, split = _rng(case, "mask"), case.kn, case.qn, max(case.split, 2)
    nkb = (kn + 31) // 32
    if case.mask == "bcast":
        m = rng.random((case.qh, 1, kn)) < 0.7
        for h in range(case.qh):
            for b in key_parts(kn, 0, split, False, True)[h % split]:
                m[h, :, b * BLOCK:(b + 1) * BLOCK] = False
        m[:, :, kn - 1] = True
        return m
    m = rng.random((1, 1, qn, kn)) < 0.7
    if nkb > 2:
        m[..., BLOCK:2 * BLOCK] = False
    for tile, part in ((qn // BLOCK - 1, 1), (qn // BLOCK - 2, 0)):
        if tile >= 0:
            for b in key_parts(kn, tile * BLOCK, split, case.causal, True)[part]:
                m[..., tile * BLOCK:(tile + 1) * BLOCK, b * BLOCK:(b + 1) * BLOCK] = False
    m[..., min(5, qn - 1), :] = False
    return m


def visibility(case, mask):
    """bool [QH, QN, KN]: key j is visible to query i iff (not causal or j <= i: aligned top-left, triton_atten.py:287-288) and the mask lets it."""
    vis = np.ones((case.qh, case.qn, case.kn), dtype=bool)
    if case.causal:
        vis &= np.arange(case.kn)[None, None, :] <= np.arange(case.qn)[None, :, None]
    if mask is not None:
        vis &= np.broadcast_to(mask if mask.ndim == 4 else mask[None], (1, case.qh, case.qn, case.kn))[0]
    return vis


def planted_positions(case, vis):
    """pos [QH, QN]: the critical key planted in every row (-1: none is visible).  Rows are numbered r = h * QN + i over the query heads and row r
    takes the next visible critical key from the r-th on, so 32 consecutive rows walk 16 key blocks and the rows of one tile have their dominant
    keys in different parts.  Under causal every fourth row takes its diagonal key i and every fourth the largest critical key <= i."""
    crit = critical_keys(case.kn)
    pos = np.full((case.qh, case.qn), -1, dtype=np.int64)
    for h in range(case.qh):
        for i in range(case.qn):
            r = (h * case.qn + i) % len(crit)
            allowed = [j for j in crit[r:] + crit[:r] if vis[h, i, j]]
            if case.causal and i % 4 == 0 and i < case.kn and vis[h, i, i]:
                pos[h, i] = i
            elif allowed:
                pos[h, i] = max(allowed) if case.causal and i % 4 == 2 else allowed[0]
    return pos


@functools.lru_cache(maxsize=4)
def inputs(case, family):
    """float32 VALUES of the case's tensors in its dtype: dict(q, k, v [Z, H, N, D], mask (bool / float32 numpy or None), vis [QH, QN, KN],
    pos [QH, QN] (family "B")).  Left unchanged by everyone: cached."""
    rng = _rng(case, family)
    z, qh, kh, qn, kn, d = case.z, case.qh, case.kh, case.qn, case.kn, case.d
    mask = build_mask(case)
    vis = visibility(case, mask)
    pos = None
    if family == "A":
        q = np.zeros((z, qh, qn, d), dtype=np.float32)
        k = O.round_dtype((rng.standard_normal((z, kh, kn, d)) + 1.0).astype(np.float32), case.tag)
        v = np.broadcast_to((np.arange(kn)[:, None] % d == np.arange(d)[None, :]).astype(np.float32), (z, kh, kn, d)).copy()
    else:
        k = O.round_dtype(rng.standard_normal((z, kh, kn, d)).astype(np.float32), case.tag)
        v = O.round_dtype(rng.standard_normal((z, kh, kn, d)).astype(np.float32), case.tag)
        q = O.round_dtype(rng.standard_normal((z, qh, qn, d)).astype(np.float32), case.tag)  # rows with no visible critical key stay random
        pos = planted_positions(case, vis)
        for h in range(qh):
            rows = np.nonzero(pos[h] >= 0)[0]
            q[:, h, rows] = O.round_dtype(3.0 * k[:, h * kh // qh, pos[h, rows]], case.tag)
    if mask is not None and case.mask != "bool":  # additive: 0 / -inf
        mask = np.where(mask, np.float32(0), np.float32(-np.inf)).astype(np.float32)
    for a in (q, k, v, vis) + ((mask,) if mask is not None else ()) + ((pos,) if pos is not None else ()):
        a.setflags(write=False)
    return dict(q=q, k=k, v=v, mask=mask, vis=vis, pos=pos)


def run_oracle(case, family, mask="own", out_tag=None, **over):
    """oracle.attention on the case's inputs; `mask`: a bool array [1, QH, QN, KN] in place of the case's own mask."""
    x = inputs(case, family)
    return O.attention(x["q"], x["k"], x["v"], case.tag, is_causal=case.causal, mask=x["mask"] if isinstance(mask, str) else mask,
                       matmul_dtype=case.mm, pv_matmul_dtype=case.pv, out_tag=out_tag, **over)


@functools.lru_cache(maxsize=4)
def planted_reference(case):
    ref = run_oracle(case, "B")
    ref.setflags(write=False)
    return ref


def census_reference(case, vis=None):
    """numpy float64: (out [Z, QH, QN, D], n_visible [QH, QN]); a row with no visible key is 0."""
    x = inputs(case, "A")
    vis = x["vis"] if vis is None else vis
    n = vis.sum(-1)
    out = np.empty((case.z, case.qh, case.qn, case.d))
    for h in range(case.qh):
        out[:, h] = (vis[h].astype(np.float64) @ x["v"][:, h * case.kh // case.qh].astype(np.float64)) / np.maximum(n[h], 1)[:, None]
    return out, n


# ---- the two assertion helpers ----------------------------------------------------------------------------------------------------------------
def census_error(got, ref, n):
    """Signed error of every (row, channel) in keys: (got - ref) * n_visible, a dead row counted as one key wide."""
    return (got.astype(np.float64) - ref) * np.maximum(n, 1)[None, :, :, None]


def assert_census(got, ref, n, label, bound=QUARTER_KEY):
    """Every row and channel within `bound` keys of the census; names the worst row, its channel and the signed key count.  Returns the worst error
    in keys."""
    err = census_error(got, ref, n)
    bad = ~(np.abs(err) <= bound)  # (NaN is bad)
    if bad.any():
        w = np.unravel_index(np.nanargmax(np.where(np.isnan(err), np.inf, np.abs(err))), err.shape)
        raise AssertionError(f"{label}: {int(bad.any(-1).sum())} rows off the key census; worst at batch {w[0]} head {w[1]} row {w[2]} channel {w[3]}: "
                             f"{err[w]:+.3f} keys of {int(n[w[1], w[2]])} visible (got {got[w]:.6g}, census {ref[w]:.6g})")
    return float(np.abs(err).max())


# the limits of tests/test_attention.py (test_hip_attention_vs_reference_kernel_and_oracle and ..._variants_...): max error / L2 error relative to the
# reference, widened for a quantized P by `_variant` there
def planted_limits(case):
    from tests.test_attention import _variant
    lim, lim2 = (1.2e-2, 4e-3) if case.tag == "bf16" else (3e-3, 1e-3)
    vlim = _variant(dict(matmul_dtype=case.mm, pv_matmul_dtype=case.pv))[2]
    if vlim is not None:
        lim, lim2 = max(lim, vlim[0]), max(lim2, vlim[1])
    return lim, lim2


def assert_planted(got, ref, lim, lim2, label):
    """max |got - ref| <= lim max|ref| and the L2 error <= lim2, as tests/test_attention.py compares with the oracle; names the worst row.  Returns
    (max error, L2 error), both relative."""
    got = got.astype(np.float64)
    diff = np.abs(got - ref)
    err, err2 = diff.max() / np.abs(ref).max(), np.linalg.norm(got - ref) / np.linalg.norm(ref)
    if not (err <= lim and err2 <= lim2):
        w = np.unravel_index(np.nanargmax(np.where(np.isnan(diff), np.inf, diff)), diff.shape)
        raise AssertionError(f"{label}: max error {err:.3e} of max|ref| (limit {lim:g}), L2 {err2:.3e} (limit {lim2:g}); worst at batch {w[0]} head {w[1]} "
                             f"row {w[2]} channel {w[3]}: got {got[w]:.6g}, oracle {ref[w]:.6g}")
    return float(err), float(err2)
