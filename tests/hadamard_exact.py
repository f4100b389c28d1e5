"""Inputs on which a Hadamard rotation cannot depend on the order of its additions, the expectation computed without the oracle's matrix
product, and the row quantizer's dispatch restated (sdnq_amd/csrc/rowquant.hip, hadamard_dev.h).

A row is i * 2^e with integers |i| <= amp and ONE exponent e per row, and g * amp <= 2^24.  Every partial sum of every butterfly order, of
the +-1/4 matrix products of the group-256 kernels and of their three-way bf16 split is then an integer multiple of 2^e (2^(e-4) on the
matrix cores) below 2^24 of it: exact in float32.  What is left is the kernels' contract, "unscaled butterflies, then * scale, then ONE
rounding to the dtype":  rotate(x)[i] = round_T(fl32(fl32(S_i) * c_T(g))),  S_i = sum_j x_j sign(H_g[j][i]),  with the signs of the
reference's own matrices (tests/golden/hadamard.npz) and c = oracle.hadamard_scale(g, T).  For power-of-4 groups c is a power of two and the
value is the reference's whatever the order; for the Sylvester groups c_T has at most 11 significant bits in the 16-bit dtypes and S * c is
exact in float32 as well; only float32 with a Sylvester group pins the contract above and not the reference's matmul -- tests/
test_hadamard_exact_host.py shows the oracle agrees there too.

Shared by tests/test_hadamard_exact_host.py (CPU) and tests/test_hadamard_exact_gpu.py.
"""
import functools
import os
import zlib

import numpy as np

from oracle import oracle as O

GROUPS = (4, 8, 16, 32, 64, 128, 256, 512)
TAGS = ("bf16", "f16", "f32")
LIMIT = {"bf16": 256, "f16": 2048, "f32": 4096}      # largest |integer| of a row: 2^(significand bits) of the 16-bit dtypes
SIG_BITS = {"bf16": 8, "f16": 11, "f32": 24}
# whole-row powers of two.  2^-70: the row scale amax / 127 has a biased exponent below 127 - 60, outside RowDiv::fast's window (sdnq_dev.h),
# so the codes of that row come from the IEEE division.  float16 stays inside its normal range: the smallest rotated magnitude is
# c(512) 2^-4 > 2^-9, the largest sqrt(512) * 2048 < 65504 without a scale, so only negative exponents are used there.
ROW_EXP = {"bf16": (-70, 3), "f16": (-4, -2), "f32": (-70, 3)}
TUNING_ENV = ("SDNQ_HIP_HADAMARD_MFMA", "SDNQ_HIP_RQ_SPLIT", "SDNQ_HIP_RQ_SPLIT2", "SDNQ_HIP_RQ_SPLIT4_NP", "SDNQ_HIP_RQH_WIDE_MIN")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hadamard.npz")


def require_default_tuning():
    """`rowquant_form` restates the launcher's own rule: with a tuning variable set the cases would run on other kernels than they claim."""
    bad = [v for v in TUNING_ENV if v in os.environ]
    assert not bad, f"unset {', '.join(bad)}: the Hadamard exactness tests need the launcher's own choice of kernel"


def is_pow4(g: int) -> bool:
    return g in (4, 16, 64, 256)


@functools.lru_cache(maxsize=None)
def sign_matrix(g: int) -> np.ndarray:
    """sign(H_g) as the reference built it (int64 [g, g], entry [j][i] multiplies x_j into y_i)."""
    with np.load(GOLDEN) as z:
        h = z[f"H{g}"].astype(np.float64)
    assert h.shape == (g, g) and np.all(np.abs(h) == np.abs(h[0, 0])) and h[0, 0] > 0, g
    return np.sign(h).astype(np.int64)


def split_rows(x: np.ndarray):
    """x [m, k] (every row an integer row times one power of two) -> (int64 [m, k], float64 2^e [m, 1]); asserted exact."""
    x = np.asarray(x, dtype=np.float64)
    mant, ex = np.frexp(x)
    i = np.rint(mant * 2.0 ** 53).astype(np.int64)
    assert np.array_equal(i.astype(np.float64) * 2.0 ** -53, mant)
    low = np.where(i == 0, np.int64(1) << 62, i & -i)
    low_exp = np.where(i == 0, 4096, ex - 53 + np.log2(low.astype(np.float64)).astype(np.int64))
    e = low_exp.min(axis=1, keepdims=True)
    e = np.where(e == 4096, 0, e)
    unit = np.exp2(e.astype(np.float64))
    ints = np.rint(x / unit).astype(np.int64)
    assert np.array_equal(ints.astype(np.float64) * unit, x), "a row is not integer * 2^e"
    return ints, unit


def int_sums(ints: np.ndarray, g: int, signs: np.ndarray | None = None) -> np.ndarray:
    """S [m, k] int64: every group of g columns times the sign matrix.  Through the float64 BLAS (numpy's int64 matmul is a scalar loop),
    exact while g * max|i| < 2^53: asserted."""
    m, k = ints.shape
    assert k % g == 0
    signs = sign_matrix(g) if signs is None else signs
    assert float(np.abs(ints).max(initial=0)) * g < 2.0 ** 53
    s = ints.astype(np.float64).reshape(m, k // g, g) @ signs.astype(np.float64)
    return np.rint(s).astype(np.int64).reshape(m, k)


def scaled_round(s: np.ndarray, unit: np.ndarray, c: float, tag: str) -> np.ndarray:
    """round_T(fl32(fl32(S 2^e) * fl32(c))): the product is ONE float32 multiplication, as the kernels' `v *= scale`."""
    assert int(np.abs(s).max(initial=0)) <= 1 << 24, "an integer sum left float32"
    s32 = (s.astype(np.float64) * unit).astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s.astype(np.float64) * unit)
    c32 = np.float32(c)
    assert float(c32) == c
    with np.errstate(under="ignore"):
        return O.round_dtype((s32 * c32).astype(np.float32), tag)


def expected_rotation(x: np.ndarray, g: int, tag: str) -> np.ndarray:
    """rotate_hadamard(x, g) on rows of `exact_rows` as float32 values of `tag`, from integer sums: no float addition takes part."""
    shape = np.shape(x)
    ints, unit = split_rows(np.asarray(x).reshape(-1, shape[-1]))
    return scaled_round(int_sums(ints, g), unit, O.hadamard_scale(g, tag), tag).reshape(shape)


def representable(v: np.ndarray, tag: str) -> np.ndarray:
    """elementwise: the float64 value is a number of `tag`."""
    with np.errstate(over="ignore", under="ignore"):
        v32 = v.astype(np.float32)
    return (v32.astype(np.float64) == v) & (O.round_dtype(v32, tag).astype(np.float64) == v)


def inexact_share(x: np.ndarray, g: int, tag: str) -> float:
    """Share of the rotated values S c (exact in float64: 24 + 24 bits) that are NOT numbers of `tag` before the rounding, over the rows
    that are not all zero.  Where it is low a rounding in the wrong place -- before the scale, twice, or none -- would not show."""
    ints, _ = split_rows(x)
    live = np.abs(ints).max(axis=1) > 0
    v = int_sums(ints[live], g).astype(np.float64) * O.hadamard_scale(g, tag)
    return float(1.0 - representable(v, tag).mean())


def rounding_can_show(g: int, tag: str) -> bool:
    """float32 with a power-of-4 group: S < 2^24 times a power of two IS a float32, the rounding is the identity for every input."""
    return not (tag == "f32" and is_pow4(g))


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _ordinary_groups(rng, n: int, g: int, tag: str, amp: int, picky: bool) -> np.ndarray:
    """n groups of g integers, magnitudes in [amp / 2, amp], random signs.  `picky`: only groups of which at least three quarters of the
    rotated values are not numbers of `tag` are kept (power-of-4 groups need |S| well above 2^significand for that: a minority of the
    draws at g = 4 and 16), drawn in batches until n are found."""
    out, have = [], 0
    batch = max(512, (1 << 20) // g)
    c = O.hadamard_scale(g, tag)
    for _ in range(4000):
        mag = rng.integers(max(amp // 2, 1), amp + 1, size=(batch, g))
        cand = mag * (rng.integers(0, 2, size=(batch, g)) * 2 - 1)
        if picky:
            v = int_sums(cand, g).astype(np.float64) * c
            cand = cand[(~representable(v, tag)).mean(axis=1) >= 0.75]
        out.append(cand)
        have += len(cand)
        if have >= n:
            return np.concatenate(out)[:n]
    raise AssertionError(f"group {g} {tag}: too few groups with enough inexact rotated values")


@functools.lru_cache(maxsize=32)
def exact_rows(m: int, k: int, tag: str, seed: int, amp: int | None = None, group: int = 0) -> np.ndarray:
    """float32 [m, k], read-only: integer rows |x| <= amp (default: the dtype's limit) times one power of two per row, representable in `tag`.
    From three rows on: row 0 is scaled by 2^ROW_EXP[tag][0] (bf16 / f32: off RowDiv::fast's window), row 1 is all zero, row 2 has a
    dominant element -- with a `group`, the group in the middle of the row holds amp * (column i0 of the sign matrix), which rotates to the
    single value amp g c at position i0 and zeros: the row's scale is set by that one position; without, one element is 32 times the
    others' limit -- and row 3 is scaled by 2^ROW_EXP[tag][1].  With a `group` at the dtype's limit at least half of the rotated values of
    the non-zero rows are not numbers of `tag` before the rounding (asserted; impossible and not asked for float32 with a power-of-4 group)."""
    limit = LIMIT[tag]
    full = amp is None or amp == limit
    amp = limit if amp is None else amp
    assert 1 <= amp <= limit and max(group, 1) * amp <= 1 << 24 and (group == 0 or (group in GROUPS and k % group == 0))
    rng = _rng("rows", m, k, tag, seed, amp, group)
    picky = bool(group) and full and rounding_can_show(group, tag)
    if group:
        ints = _ordinary_groups(rng, m * (k // group), group, tag, amp, picky).reshape(m, k)
    else:
        ints = rng.integers(-amp, amp + 1, size=(m, k))
    exps = np.zeros(m, dtype=np.int64)
    if m >= 3:
        ints[1::5] = 0
        for r in range(2, m, 5):
            if group:
                mid, i0 = (k // group) // 2, int(rng.integers(0, group))
                ints[r, mid * group:(mid + 1) * group] = amp * sign_matrix(group)[:, i0]
            else:
                ints[r] = np.clip(ints[r], -(amp // 32), amp // 32)
                ints[r, int(rng.integers(0, k))] = -amp
        exps[0::5] = ROW_EXP[tag][0]
        exps[3::5] = ROW_EXP[tag][1]
    x = ints.astype(np.float64) * np.exp2(exps.astype(np.float64))[:, None]
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x) and np.array_equal(O.round_dtype(x32, tag), x32), "a row is not representable"
    if group:
        rot = np.abs(int_sums(ints, group))
        for r in (range(2, m, 5) if m >= 3 else ()):
            assert (rot[r] == rot[r].max()).sum() == 1 and rot[r].max() == amp * group, "the dominant position is not alone"
        if picky:
            share = inexact_share(x32, group, tag)
            assert share >= 0.5, (m, k, tag, group, "inexact share", share)
    x32.setflags(write=False)
    return x32


def one_hot_rows(g: int, tag: str, k: int | None = None) -> np.ndarray:
    """float32 [g, k]: row r holds the integer v_r != 0 at column (k - g) + r, the LAST group of the row: rotated, that group of row r is
    v_r times row r of the sign matrix times c -- every sign of every column of the kernel's rotation, one by one."""
    k = g if k is None else k
    v = (np.arange(g) % 7 + 1) * np.where(np.arange(g) % 3 == 0, -1, 1)
    x = np.zeros((g, k), dtype=np.float32)
    x[np.arange(g), k - g + np.arange(g)] = v
    return x


# ------------------------------------------------------------------------------------------------
# the dispatcher of sdnq_hip_rowquant / rowquant_lp_impl (rowquant.hip), restated
# ------------------------------------------------------------------------------------------------
def rowquant_form(m: int, k: int, tag: str, group: int = 0, asym: bool = False, lp: bool = False, prefetch: bool = False) -> str:
    """The kernel and template cell a row-quantizer call lands on under default tuning:
      had256-NG{4,8,12,16}-W{1,4}   rowquant_had256_kernel<T, MM, NG, WPR> (group 256 on the matrix cores)
      {fwht,plain}-NP{2,3,5,10}-W1  rowquant_kernel<T, MM, HAD, NP>: the row in registers, one wave per row
      {fwht,plain}-NP{2,3,8}-W4     ... four waves per row
      {fwht,plain}-NP0              the two-phase form for rows past the register cache
      {fwht,plain}-NP0-LP           rowquant_lp / rowquant_lp_asym (always two-phase)
    `prefetch`: a prefetch tensor is passed (its workgroups ride along; rows are then never split).  (x and xq are torch allocations: the
    alignment conditions of the matrix-core route always hold.)"""
    require_default_tuning()
    assert m > 0 and k > 0 and k % 8 == 0 and tag in TAGS
    assert group == 0 or (group in GROUPS and k % group == 0)
    kind = "fwht" if group else "plain"
    if lp:
        assert tag != "f32" and not prefetch
        return f"{kind}-NP0-LP"
    if group == 256 and tag != "f32" and not asym and k <= 16384:
        groups = k // 256
        wide = groups > 16 or (m <= 1024 and groups >= 8 and -(-groups // 4) * 3 < groups)
        per = -(-groups // 4) if wide else groups
        ng = 4 if per <= 4 else (8 if per <= 8 else (12 if per <= 12 else 16))
        return f"had256-NG{ng}-W{4 if wide else 1}"
    np_ = -(-k // 512)
    can_split = m <= 2048 and np_ >= 3 and not prefetch
    long4 = 10 < np_ <= 32 and not prefetch
    split4 = long4 or (can_split and np_ <= 12 and np_ >= 7)      # SDNQ_HIP_RQ_SPLIT4_NP = 7; two-wave rows are off (SDNQ_HIP_RQ_SPLIT2 = 0)
    if split4:
        return f"{kind}-NP{1 if np_ <= 4 else (2 if np_ <= 8 else (3 if np_ <= 12 else 8))}-W4"
    if np_ > 10:
        return f"{kind}-NP0"
    return f"{kind}-NP{2 if np_ <= 2 else (3 if np_ <= 3 else (5 if np_ <= 5 else 10))}-W1"


# ------------------------------------------------------------------------------------------------
# the case tables of tests/test_hadamard_exact_gpu.py (the host test checks that they name every reachable form)
# ------------------------------------------------------------------------------------------------
# (b) rowquant_had256_kernel: (form, m, K).  groups = K / 256; wide = groups > 16 || (m <= 1024 && groups >= 8 && ceil(groups / 4) * 3 < groups);
#     per = wide ? ceil(groups / 4) : groups;  NG = 4 | 8 | 12 | 16 for per <= 4 | 8 | 12 | else
HAD256_CASES = (
    ("had256-NG4-W1", 5, 256),       # 1 group: three of the wave's four group registers are dead
    ("had256-NG4-W1", 5, 768),       # 3 groups
    ("had256-NG8-W1", 5, 1280),      # 5 groups < 8: not wide
    ("had256-NG12-W1", 5, 2304),     # 9 groups: ceil(9 / 4) * 3 = 9 is not < 9, not wide
    ("had256-NG16-W1", 1025, 3328),  # 13 groups: wide up to 1024 rows (4 * 3 = 12 < 13), one wave per row only above; the last workgroup has one row
    ("had256-NG4-W4", 3, 2048),      # 8 groups, 2 per wave
    ("had256-NG4-W4", 3, 2560),      # 10 groups, per = 3: waves hold 3, 3, 3, 1
    ("had256-NG8-W4", 3, 4352),      # 17 groups > 16, per = 5: 5, 5, 5, 2
    ("had256-NG12-W4", 3, 8448),     # 33 groups, per = 9: 9, 9, 9, 6
    ("had256-NG16-W4", 3, 12544),    # 49 groups, per = 13: 13, 13, 13, 10
    ("had256-NG16-W4", 3, 16384),    # 64 groups: every register of every wave live, the last K of the route
)
# (c) / (d) rowquant_kernel: (form without its fwht- / plain- prefix, m, K, prefetch).  np = ceil(K / 512); four waves per row for
#     7 <= np <= 12 (m <= 2048, no prefetch) and for 11 <= np <= 32 (no prefetch); W4 NP = 2 | 3 | 8 for np <= 8 | 12 | else;
#     one wave: NP = 2 | 3 | 5 | 10 for np <= 2 | 3 | 5 | 10, else the two-phase form
ROWQUANT_CASES = (
    ("NP2-W1", 5, 520, False),       # np = 2, the second pass holds one lane (8 elements); group 8 and 4 only (520 = 8 * 65)
    ("NP2-W1", 5, 1024, False),      # np = 2, both passes full: the only K of this form that takes group 512
    ("NP3-W1", 5, 1536, False),      # np = 3
    ("NP5-W1", 5, 2560, False),      # np = 5
    ("NP10-W1", 5, 3072, False),     # np = 6 < 7: passes 6..9 of the ten lie past the row
    ("NP10-W1", 5, 3584, True),      # np = 7 would split, a prefetch tensor forbids it: row workgroups + prefetch workgroups
    ("NP2-W4", 3, 3584, False),      # np = 7: waves hold 1024, 1024, 1024, 512
    ("NP3-W4", 3, 5120, False),      # np = 10: 1536, 1536, 1536, 512
    ("NP3-W4", 3, 6144, False),      # np = 12: every wave full
    ("NP8-W4", 3, 6656, False),      # np = 13: 4096, 2560, and waves 2 and 3 wholly past the row
    ("NP8-W4", 3, 16384, False),     # np = 32: every wave full
    ("NP0", 3, 16896, False),        # np = 33 > 32: two-phase
)
LP_CASES = (("NP0-LP", 5, 768), ("NP0-LP", 3, 5632))


def groups_of(k: int):
    return tuple(g for g in GROUPS if k % g == 0)


def fwht_configs(m: int, k: int, prefetch: bool):
    """The (tag, group, mode) runs of one (c) shape: every dtype with each of symmetric int8 + rowsum, fp8 and asymmetric, the groups dealt
    round so that over the table every group meets every dtype -- never a combination that leaves for the matrix cores (group 256 on 16-bit
    symmetric rows up to K = 16384)."""
    gs = groups_of(k)
    out = []
    for i, (tag, mode) in enumerate((t, md) for t in TAGS for md in ("int8", "fp8", "asym")):
        for step in range(len(gs)):
            g = gs[(i + k // 512 + step) % len(gs)]
            if rowquant_form(m, k, tag, g, mode == "asym", False, prefetch).startswith("fwht"):
                out.append((tag, g, mode))
                break
    # group 256 wherever this kernel takes it: float32 rows, asymmetric 16-bit rows, any row past 16384
    if 256 in gs:
        for tag, mode in (("f32", "int8"), ("bf16", "asym"), ("f16", "asym")) + ((("bf16", "int8"), ("f16", "fp8")) if k > 16384 else ()):
            if (tag, 256, mode) not in out:
                out.append((tag, 256, mode))
    return tuple(out)


def all_case_forms():
    """Every form the GPU file's tables claim to run, by `rowquant_form` on the tables' own shapes."""
    forms = set()
    for _, m, k in HAD256_CASES:
        forms |= {rowquant_form(m, k, tag, 256) for tag in ("bf16", "f16")}
    for _, m, k, pf in ROWQUANT_CASES:
        forms |= {rowquant_form(m, k, tag, g, mode == "asym", False, pf) for tag, g, mode in fwht_configs(m, k, pf)}
        forms.add(rowquant_form(m, k, "bf16", 0, False, False, pf))
    for _, m, k in LP_CASES:
        forms |= {rowquant_form(m, k, "bf16", g, asym, True) for g in (0, 256) for asym in (False, True)}
    return forms
