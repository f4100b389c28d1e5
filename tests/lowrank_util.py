"""Inputs and CPU expected values of the bit-exact tests of the many-row SVD branch: sdnq_hip_lowrank_down and the low-rank epilogue
of the int8 / fp8 GEMM (tests/test_lowrank_exact_gpu.py, tests/test_lowrank_exact_host.py).

The low-rank factors t [M,R] and svd_up [N,R] are exact-sum operands (tests/exact_inputs.py: small integers times one power of two per
row), the bias an integer in the units of every low-rank sum: bias + t . up^T is then exact in float32 in every summation order -- the
MFMAs of the staged paths, the sequential fmaf chain, a double sum on the CPU -- and bias2d = cast_svd(that) is ONE rounding of an exact
value.  The main product is exact too (int32 sums of int8 codes; exact-sum e4m3 operands), so every output element has exactly one
correct bit pattern and the comparison is np.array_equal.

The scales follow the row exponents of the factors, so that in EVERY row the scaled accumulator and bias2d have the same order of
magnitude: the output's rounding cannot swallow a low-rank term that went missing (sensitivity(), enforced by the builder).
"""
import functools
import os
from dataclasses import dataclass

import numpy as np
import torch

from oracle import oracle as O
from tests import exact_inputs as X

TUNING_VARS = ("SDNQ_HIP_TILE", "SDNQ_HIP_TILE_MAP", "SDNQ_HIP_TALL_MIN_TILES", "SDNQ_HIP_LRD_RT")
TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
DT = X.TAG_DT

SMALL_SHAPES = ((300, 392, 528), (257, 264, 48), (513, 1288, 208), (33, 72, 16))
# the smallest shapes the launcher sends to the 256x256 EPI_LRFAST tiles: 10 x 16 = 160 tiles, a tail of 4 rows and one of 8 columns
LRFAST_SHAPES = ((2308, 3848, 2048), (2308, 3848, 2064))
# forced tile ids of a low-rank launch: 1 = 64x128, 2 = 64x64, 3 = 256x128 (0 is the same kernel as 3; ids >= 4 exist for the plain
# epilogues only, PP_OK in gemm.hip); -1 = the heuristics
TILES = (1, 2, 3, -1)


def require_default_tuning():
    """The case tables name the kernel the LAUNCHER picks; a tuning variable would send a case to another kernel than it claims."""
    for var in TUNING_VARS:
        assert var not in os.environ, f"unset {var}: the low-rank cases need the launcher's own choices"


# ---- the launcher's rules, restated (gemm.hip: gemm_kernel's epilogue dispatch and launch_tiles; linear_float.hip) -----------------
REGISTER, STAGED_LDS, STAGED_GLOBAL, FMAF = "register layout", "staged, factors in LDS", "staged, fragments from global", "fmaf chain"


def epilogue_path(rank: int, svd: str, out: str, zero_point: bool = False) -> str:
    """lr_mfma = rank % 16 == 0 && svd dtype != f32; lr_lds = lr_mfma && rank == 32; the register layout needs lr_lds, no zero-point
    term, a 16-bit output and svd dtype == output dtype."""
    if rank % 16 != 0 or svd == "f32":
        return FMAF
    if rank != 32:
        return STAGED_GLOBAL
    if out != "f32" and svd == out and not zero_point:
        return REGISTER
    return STAGED_LDS


def takes_lrfast(m: int, n: int, k: int, rank: int, svd: str, out: str, zero_point: bool = False) -> bool:
    """launch_tiles<.., EPI_LOWRANK>: tiles(256, 256) >= 160 && K >= 2048 && rank == 32 && svd dtype == output dtype (16 bits) && no
    zero-point term -> the 256x256 tile with EPI_LRFAST (register layout in two chunks)."""
    tiles = -(-m // 256) * -(-n // 256)
    return tiles >= 160 and k >= 2048 and rank == 32 and out != "f32" and svd == out and not zero_point


def lrfast_ring(k: int) -> str:
    """ht_ok: K % 128 == 0 and 32-bit row offsets -> the half-tile ring (LD_HT), else the 64-byte software pipeline (LD_PIPE)."""
    return "half-tile ring" if k % 128 == 0 and 256 * k + k < 2 ** 31 else "64-byte pipeline"


def default_tile(m: int, n: int, rank: int = 32, svd: str = "bf16", out: str = "bf16", k: int = 16) -> tuple:
    """The tile of a low-rank launch under the heuristics (no ping-pong configurations: PP_OK is false for EPI_LOWRANK)."""
    if takes_lrfast(m, n, k, rank, svd, out):
        return (256, 256)
    if m >= 2048 and -(-m // 256) * -(-n // 128) >= 230:
        return (256, 128)
    return (64, 128) if m > 128 else (64, 64)


def lrd_row_tiles(m: int) -> int:
    """sdnq_hip_lowrank_down: RT = 2 when two 16-row tiles per workgroup leave the busiest of 256 CUs fewer bytes to move."""
    wg1, wg2 = -(-m // 16), -(-m // 32)
    return 2 if -(-wg2 // 256) * 4 < -(-wg1 // 256) * 3 else 1


# (rank, svd dtype, output dtype) per run-time path of the low-rank epilogue; epilogue_path() must name the path for each
COMBOS = (
    (REGISTER, 32, "bf16", "bf16"), (REGISTER, 32, "f16", "f16"),
    (STAGED_LDS, 32, "bf16", "f32"), (STAGED_LDS, 32, "f16", "f32"), (STAGED_LDS, 32, "bf16", "f16"),
    (STAGED_GLOBAL, 16, "bf16", "bf16"), (STAGED_GLOBAL, 16, "f16", "f16"), (STAGED_GLOBAL, 48, "bf16", "bf16"), (STAGED_GLOBAL, 48, "f16", "f16"),
    (STAGED_GLOBAL, 64, "bf16", "bf16"), (STAGED_GLOBAL, 64, "f16", "f16"),
    (FMAF, 8, "bf16", "bf16"), (FMAF, 8, "f16", "f16"), (FMAF, 24, "bf16", "bf16"), (FMAF, 24, "f16", "f16"), (FMAF, 40, "bf16", "bf16"),
    (FMAF, 40, "f16", "f16"), (FMAF, 32, "f32", "f32"), (FMAF, 32, "f32", "bf16"),
)


def combo_id(c) -> str:
    return f"{c[0].replace(', ', '-').replace(' ', '_')}-r{c[1]}-{c[2]}-{c[3]}"


# ---- operands ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Main:
    mm: str
    a: torch.Tensor        # [m, k] int8 | float8_e4m3fn
    b: torch.Tensor        # [n, k]
    ints: np.ndarray       # int64 [m, n]: the accumulators in units of 2^(ea[m] + eb[n])
    ea: np.ndarray
    eb: np.ndarray

    @property
    def acc(self) -> np.ndarray:
        return self.ints.astype(np.float64) * np.exp2((self.ea[:, None] + self.eb[None, :]).astype(np.float64))

    def codes(self):
        if self.mm == "int8":
            return self.a.numpy(), self.b.numpy()
        return self.a.view(torch.uint8).numpy(), self.b.view(torch.uint8).numpy()


@functools.lru_cache(maxsize=None)
def main_operands(mm: str, m: int, n: int, k: int, zero: bool = False) -> Main:
    """int8: any codes in [-127, 127] (the int32 accumulator is exact); fp8: exact-sum e4m3 operands.  zero=True: all-zero activations
    (the factor census)."""
    if mm == "int8":
        rng = np.random.default_rng(m + 3 * n + 5 * k)
        ia = np.zeros((m, k), dtype=np.int64) if zero else rng.integers(-127, 128, size=(m, k))
        ib = rng.integers(-127, 128, size=(n, k))
        z = np.zeros
        return Main(mm, torch.from_numpy(ia.astype(np.int8)), torch.from_numpy(ib.astype(np.int8)), X.int_matmul(ia, ib), z(m, np.int64), z(n, np.int64))
    ex = X.exact_operands(m, n, k, seed=m + n + k, fmt="fp8")
    if zero:
        return Main(mm, torch.zeros_like(ex.a), ex.b, np.zeros((m, n), dtype=np.int64), ex.ea, ex.eb)
    return Main(mm, ex.a, ex.b, X.expected_int(ex.ia, ex.ib), ex.ea, ex.eb)


def factor_tensor(vals: torch.Tensor, svd: str) -> torch.Tensor:
    """16-bit exact-sum values in the svd dtype (float32 factors hold the same bf16 values)."""
    return vals.float() if svd == "f32" else vals


def round_to(a: np.ndarray, tag: str) -> np.ndarray:
    """float64 values that float32 holds -> rounded ONCE to `tag`, as float32."""
    a32 = a.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a), "not an exact float32 value: the rounding to the target would be a second one"
    return torch.from_numpy(np.ascontiguousarray(a32)).to(DT[tag]).float().numpy()


def _rb(a) -> np.ndarray:
    return O.round_dtype(np.asarray(a, dtype=np.float32), "bf16")


def restated_epilogue(acc, sa, sb, bias, tag: str, lp: bool = False, rowsum=None, zp=None, a_zp=None, wcs=None, k: int = 0) -> np.ndarray:
    """The scaled matmul's epilogue with the zero-point terms of unsigned weights (linear_int8.py:57-69) and of the uint8 matmul
    (linear_uint8.py:61-66), op by op in float32 as the kernel comments of gemm.hip cite them:
        vv   = f32(acc) * sa
        zsum = f32(rowsum) * sa;  zb = zsum * zp                         sum(input).to(scale dtype).mul_(input_scale).mul(zero_point)
        zb   = zb + wcs * a_zp                                           + colsum(w) * ws * xzp
        zb   = fma(a_zp * zp, K, zb)                                     zero_bias.add_(mul(xzp, wzp), alpha=K): ONE fused multiply-add
        bv   = zb + bias2d                                               zero_bias.add_(bias)
        out  = cast(fma(vv, sb, bv))                                     addcmul: one rounding
    lp: the same chain on bfloat16 tensors (sdnq_hip_scaled_mm_lp, _lp_zp, _lp_uzp[_svd]) -- every op's float32 result is rounded to
    bf16, the conversions of the int32 accumulator and row sum included.  bias: None | [N] | [M, N] float32 (the low-rank bias2d)."""
    f = np.float32
    r = _rb if lp else (lambda v: v)
    a32 = np.asarray(acc).astype(f)
    assert np.array_equal(a32.astype(np.float64), acc), "accumulators must be float32 values"
    sa = np.asarray(sa, dtype=f).reshape(-1, 1)
    sb = np.asarray(sb, dtype=f).reshape(1, -1)
    vv = r(r(a32) * sa)
    zb = None
    if zp is not None:
        zp = np.asarray(zp, dtype=f).reshape(1, -1)
        zsum = r(r(np.asarray(rowsum).astype(f)).reshape(-1, 1) * sa)
        zb = r(zsum * zp)
    if a_zp is not None:
        a_zp = np.asarray(a_zp, dtype=f).reshape(-1, 1)
        t2 = r(np.asarray(wcs, dtype=f).reshape(1, -1) * a_zp)
        zb = t2 if zb is None else r(zb + t2)
        if zp is not None:
            zb = r(X._fma_f32(r(a_zp * zp), np.full((1, 1), k, dtype=f), zb))
    bv = None
    if bias is not None:
        bias = np.asarray(bias, dtype=f)
        bv = bias.reshape(1, -1) if bias.ndim == 1 else bias
    if zb is not None:
        bv = zb if bv is None else r(zb + bv)
    res = vv * sb if bv is None else X._fma_f32(vv, np.broadcast_to(sb, vv.shape), np.broadcast_to(bv, vv.shape))
    return torch.from_numpy(np.ascontiguousarray(res.astype(f))).to(DT[tag]).float().numpy()


@dataclass
class Case:
    main: Main
    lr: X.Exact            # lr.a = t [m, r], lr.b = svd_up [n, r]: 16-bit exact-sum values
    bias: np.ndarray       # float32 [n], an integer in the units of every low-rank sum of its column
    sa: np.ndarray
    sb: np.ndarray
    svd: str
    out: str
    lp: bool
    zero: dict             # the zero-point operands (numpy), empty without
    share: float           # sensitivity(): the smallest share found

    @property
    def shape(self):
        return (self.main.a.shape[0], self.main.b.shape[0], self.main.a.shape[1])

    @property
    def rank(self):
        return self.lr.a.shape[1]

    def t(self) -> torch.Tensor:
        return factor_tensor(self.lr.a, self.svd)

    def up(self) -> torch.Tensor:
        return factor_tensor(self.lr.b, self.svd)

    def lowrank_f64(self, with_bias: bool) -> np.ndarray:
        """bias + t . up^T as exact float64 values."""
        s = self.lr.acc()
        return s + self.bias.astype(np.float64)[None, :] if with_bias else s

    def bias2d(self, with_bias: bool) -> np.ndarray:
        """cast_svd(bias + t . up^T): the float64 sum rounded once."""
        return round_to(self.lowrank_f64(with_bias), self.svd)

    def bias2d_oracle(self, with_bias: bool) -> np.ndarray:
        t, up = self.lr.codes()
        return O.lowrank_bias(t, up, self.bias if with_bias else None, self.svd)

    def finish(self, bias2d) -> np.ndarray:
        """The output for a given [M, N] bias (float32 holding values of the output dtype)."""
        if not self.zero and not self.lp:
            return X.epilogue(self.main.acc, self.sa, self.sb, bias2d, self.out)
        return restated_epilogue(self.main.acc, self.sa, self.sb, bias2d, self.out, self.lp, k=self.shape[2], **self.zero)

    def expected(self, with_bias: bool) -> np.ndarray:
        return self.finish(self.bias2d(with_bias))

    def expected_oracle(self, with_bias: bool) -> np.ndarray:
        """The C oracle's answer (plain forms only): lowrank_bias, then scaled_mm / scaled_mm_lp with the 2-D bias."""
        assert not self.zero
        a, b = self.main.codes()
        fn = O.scaled_mm_lp if self.lp else O.scaled_mm
        return fn(self.main.mm, a, b, self.sa, self.sb, self.bias2d_oracle(with_bias), self.out)


def sensitivity(case: Case, with_bias: bool, rows=None) -> float:
    """Zero ONE rank column of t over a 32-row block: the smallest share, over all columns and all rows (of `rows`), of the outputs of
    a row that change.  (Zeroing column c in one block changes only that block's rows, each as zeroing it everywhere would: one pass
    per column covers every block.)"""
    rows = slice(None) if rows is None else rows
    base = case.lowrank_f64(with_bias)
    sub = Case(Main(case.main.mm, case.main.a[rows], case.main.b, case.main.ints[rows], case.main.ea[rows], case.main.eb), case.lr,
               case.bias, case.sa[rows], case.sb, case.svd, case.out, case.lp, {k: (v[rows] if k in ("rowsum", "a_zp") else v) for k, v in case.zero.items()}, 0.0)
    base = base[rows]
    out0 = sub.finish(round_to(base, case.svd))
    ti = case.lr.ia[rows].astype(np.float64) * np.exp2(case.lr.ea[rows].astype(np.float64))[:, None]
    ui = case.lr.ib.astype(np.float64) * np.exp2(case.lr.eb.astype(np.float64))[:, None]
    worst = 1.0
    for c in range(case.rank):
        out_c = sub.finish(round_to(base - ti[:, c:c + 1] * ui[:, c][None, :], case.svd))
        worst = min(worst, float((out_c != out0).mean(axis=1).min()))
    return worst


SENSITIVITY_FLOOR = 0.5
SENSITIVITY_WORK = 1_000_000   # outputs x rank columns one check may recompute (about a tenth of a second)


def sample_rows(m: int, n: int, rank: int):
    """The rows a case's sensitivity is checked on: all of them while m n rank fits SENSITIVITY_WORK, else every step-th row and the
    last eight.  (Every row is drawn the same way -- its own exponent, scale and integers -- so a sample speaks for the rest; the
    check costs one epilogue per rank column and the suite pays it on every run.)"""
    if m * n * rank <= SENSITIVITY_WORK:
        return None
    step = -(-m * n * rank // SENSITIVITY_WORK)
    return np.unique(np.concatenate([np.arange(0, m, step), np.arange(max(0, m - 8), m)]))


def _scales(main: Main, lr: X.Exact, lp: bool, seed: int):
    """sa[m] ~ 2^(lr.ea[m] - main.ea[m]), sb[n] ~ 2^(lr.eb[n] - main.eb[n]), times one factor that brings the median |acc sa sb| to the
    median |t . up^T|: both terms are then comparable in EVERY row and column.  Arbitrary float32 significands; lp: powers of two (the
    bf16 chain's two multiplications are then exact, as in test_fp8_bf16_scale_chain_bit_exact_vs_oracle)."""
    rng = np.random.default_rng(seed)
    m, n = main.ints.shape
    med_main = max(float(np.median(np.abs(main.ints))), 1.0)
    med_lr = max(float(np.median(np.abs(X.expected_int(lr.ia, lr.ib)))), 1.0)
    g = med_lr / med_main
    if lp:
        g, u, v = np.exp2(np.round(np.log2(g))), np.ones(m), np.ones(n)
    else:
        u, v = rng.uniform(0.75, 1.5, size=m), rng.uniform(0.75, 1.5, size=n)
    sa = (u * g * np.exp2((lr.ea - main.ea).astype(np.float64))).astype(np.float32)
    sb = (v * np.exp2((lr.eb - main.eb).astype(np.float64))).astype(np.float32)
    return sa, sb


def _zero_terms(form: str, main: Main, lr: X.Exact, sa, sb, lp: bool, seed: int) -> dict:
    """The zero-point operands of `form`, sized so that each term is of the order of bias2d: rowsum = the true row sums of the codes,
    zp / a_zp arbitrary float32 (lp: bf16 values), wcs = f32(column sums of the weight codes) * sb (lp: rounded twice, as it arrives)."""
    if form == "":
        return {}
    assert main.mm == "int8"
    rng = np.random.default_rng(seed)
    f = np.float32
    r = _rb if lp else (lambda v_: np.asarray(v_, dtype=f))
    m, n = main.ints.shape
    a, b = main.codes()
    unit_m, unit_n = np.exp2(lr.ea.astype(np.float64)), np.exp2(lr.eb.astype(np.float64))
    out = {}
    terms = form.split("+")
    if "zp" in terms:
        rowsum = a.astype(np.int64).sum(1).astype(np.int32)
        rs = max(float(np.median(np.abs(rowsum))), 1.0)
        # zsum * zp = rowsum * sa * zp: sa carries 2^ea[m], zp carries 2^eb[n] and the size
        g = float(np.median(sa.astype(np.float64) / unit_m))
        out["rowsum"] = rowsum
        out["zp"] = r(rng.uniform(4.0, 16.0, size=n) * rng.choice([-1.0, 1.0], size=n) * unit_n / (rs * g))
    if "azp" in terms:
        colsum = b.astype(np.int64).sum(1)
        wcs = r(r(colsum.astype(f)) * sb)
        cs = max(float(np.median(np.abs(wcs.astype(np.float64) / unit_n))), 1e-30)
        out["wcs"] = wcs
        out["a_zp"] = r(rng.uniform(4.0, 16.0, size=m) * rng.choice([-1.0, 1.0], size=m) * unit_m / cs)
    return out


ZERO_FORMS = ("rowsum+zp", "azp", "azp+zp")   # uint8 weights on the int8 matmul; the uint8 matmul without / with a weight zero point


@functools.lru_cache(maxsize=None)
def make_case(mm: str, m: int, n: int, k: int, rank: int, svd: str, out: str, lp: bool = False, zero_form: str = "", check: bool = True) -> Case:
    """One case of the GEMM epilogue tests.  Draws the factors again (up to 4 times) until the sensitivity condition holds, then raises.
    check=False skips that (model-size shapes check a sample of rows themselves)."""
    fmt = "bf16" if svd == "f32" else svd
    main = main_operands(mm, m, n, k)
    why = ""
    for attempt in range(4):
        seed = 16 + 1000 * attempt + rank
        lr = X.exact_operands(m, n, rank, seed=seed, fmt=fmt, density=1.0, e_window=(-6, -1))
        bias = X.exact_bias(lr, seed + 1)
        sa, sb = _scales(main, lr, lp, seed + 2)
        case = Case(main, lr, bias, sa, sb, svd, out, lp, _zero_terms(zero_form, main, lr, sa, sb, lp, seed + 3), 1.0)
        if check:
            rows = sample_rows(m, n, rank)
            case.share = min(sensitivity(case, True, rows), sensitivity(case, False, rows))
            if case.share < SENSITIVITY_FLOOR:
                why = f"a row keeps {1 - case.share:.2f} of its outputs when a rank column goes missing"
                continue
        return case
    raise ValueError(f"make_case({mm}, {m}, {n}, {k}, rank {rank}, {svd} -> {out}, lp={lp}, {zero_form!r}): {why}")


# ---- census operands: one product per output ---------------------------------------------------------------------------------------
def window_values(rng, shape, fmt: str) -> torch.Tensor:
    """Arbitrary sign and significand, exponent in [-3, 3]: nonzero, and a product of two neither overflows nor goes subnormal in f16
    or bf16.  A product of two such values is exact in float32 (8 + 8 significand bits for bf16, 11 + 11 for f16)."""
    v = rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape)) * np.exp2(rng.integers(-3, 4, size=shape))
    t = torch.from_numpy(v.astype(np.float32)).to(X.TORCH_DT["bf16" if fmt == "f32" else fmt])
    return t.float() if fmt == "f32" else t


def one_hot_rows(dense: torch.Tensor, cols: np.ndarray) -> torch.Tensor:
    """`dense` with everything but column cols[i] of row i zeroed."""
    keep = torch.zeros(dense.shape, dtype=torch.bool)
    keep[torch.arange(dense.shape[0]), torch.from_numpy(cols)] = True
    return torch.where(keep, dense, torch.zeros_like(dense))


def factor_census(m: int, n: int, rank: int, shift: int, svd: str, transposed: bool, seed: int = 0):
    """(t, svd_up, products [m, n] float32).  The rows of t are one-hot at rank column (row + shift) % rank and svd_up is dense
    (transposed: the rows of svd_up are one-hot, t is dense), so the low-rank sum of every output is ONE product."""
    rng = np.random.default_rng(seed * 7919 + rank)   # the same dense values for every shift
    t, up = window_values(rng, (m, rank), svd), window_values(rng, (n, rank), svd)
    if transposed:
        cols = (np.arange(n) + shift) % rank
        up = one_hot_rows(up, cols)
        prod = t.float()[:, torch.from_numpy(cols)] * up.float()[torch.arange(n), torch.from_numpy(cols)][None, :]
    else:
        cols = (np.arange(m) + shift) % rank
        t = one_hot_rows(t, cols)
        prod = t.float()[torch.arange(m), torch.from_numpy(cols)][:, None] * up.float()[:, torch.from_numpy(cols)].T
    return t, up, prod


def census_expected(prod: torch.Tensor, svd: str, out: str) -> torch.Tensor:
    """cast_out(cast_svd(product)) in the output dtype: with zero activations and no bias nothing else reaches the output."""
    return prod.to(DT[svd]).to(DT[out])


# ---- lowrank_down --------------------------------------------------------------------------------------------------------------------
# (M, K, R): see the docstring of tests/test_lowrank_exact_gpu.py
DOWN_SHAPES = ((5, 16, 8), (33, 48, 8), (16, 128, 32), (100, 192, 16), (257, 400, 48), (77, 2048, 64), (64, 112, 40), (4100, 272, 32),
               (8192, 144, 32))
DOWN_MFMA = {"bf16": "bf16_16x16x32", "f16": "f16_16x16x32"}   # keys of X.MEASURED_SPAN_BITS / X.B


@functools.lru_cache(maxsize=None)
def down_case(m: int, k: int, r: int, fmt: str) -> tuple:
    """(exact-sum x [m, k] and svd_down [r, k], expected t = round_T(float64 sum) as float32)."""
    ex = X.exact_operands(m, r, k, seed=m + 3 * k + r, fmt=fmt)
    assert ex.span_bits <= X.B[DOWN_MFMA[fmt]], "span beyond the budget measured for v_mfma_f32_16x16x32"
    return ex, round_to(ex.acc(), fmt)


def down_census(m: int, k: int, r: int, shift: int, stride: int, fmt: str, transposed: bool, seed: int = 0):
    """(x, svd_down, expected t in the dtype).  x is one-hot (1.0 at column (row * stride + shift) % K) and svd_down dense and arbitrary:
    t[m][r] is svd_down[r][that column], bit for bit.  transposed: the rows of svd_down are one-hot, t[m][r] = x[m][column of r]."""
    assert stride % 2 == 1
    rng = np.random.default_rng(seed * 104729 + k)
    dt = DT[fmt]
    x = X._arbitrary(rng, (m, k), fmt) if fmt != "f32" else torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32))
    down = X._arbitrary(rng, (r, k), fmt) if fmt != "f32" else torch.from_numpy(rng.standard_normal((r, k)).astype(np.float32))
    if transposed:
        cols = (np.arange(r) * stride + shift) % k
        down = one_hot_rows(torch.ones((r, k), dtype=dt), cols)
        want = x[:, torch.from_numpy(cols)].contiguous()
    else:
        cols = (np.arange(m) * stride + shift) % k
        x = one_hot_rows(torch.ones((m, k), dtype=dt), cols)
        want = down[:, torch.from_numpy(cols)].T.contiguous()
    return x, down, want


def bits(t: torch.Tensor) -> np.ndarray:
    """The bit patterns of a float tensor (so that -0.0 and 0.0, or two NaNs, compare as what they are)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def where(got: np.ndarray, ref: np.ndarray) -> str:
    """How many differ, where, and the first differing (m, n) with both values."""
    bad = np.argwhere(got != ref)
    if len(bad) == 0:
        return "equal"
    return f"{len(bad)} of {ref.size} differ, rows {bad[:, 0].min()}..{bad[:, 0].max()}, columns {bad[:, 1].min()}..{bad[:, 1].max()}, " \
           f"first (m, n) = {tuple(int(i) for i in bad[0])}: got {got[tuple(bad[0])]!r} want {ref[tuple(bad[0])]!r}"


# ---- modelled faults (tests/test_lowrank_exact_host.py): what a subtly wrong kernel would write -------------------------------------
def _factors_f64(case: Case):
    t = case.lr.ia.astype(np.float64) * np.exp2(case.lr.ea.astype(np.float64))[:, None]
    up = case.lr.ib.astype(np.float64) * np.exp2(case.lr.eb.astype(np.float64))[:, None]
    return t, up


def _with_factors(case: Case, t: np.ndarray, up: np.ndarray, with_bias: bool) -> np.ndarray:
    s = t @ up.T   # float64: sums of at most 1024 products of small integers times powers of two, exact
    if with_bias:
        s = s + case.bias.astype(np.float64)[None, :]
    return case.finish(round_to(s, case.svd))


def fault_drop_rank_column(case: Case, block: int, col: int, with_bias: bool):
    """A rank column lost in one 32-row block: (output, rows touched)."""
    t, up = _factors_f64(case)
    rows = np.arange(block * 32, min(case.shape[0], block * 32 + 32))
    t[rows, col] = 0.0
    return _with_factors(case, t, up, with_bias), rows


def fault_swap_rank_halves(case: Case, step: int, with_bias: bool):
    """The two 8-element halves of 16-rank MFMA step `step` of t read in each other's place (svd_up as it is)."""
    t, up = _factors_f64(case)
    k0 = step * 16
    t[:, k0:k0 + 8], t[:, k0 + 8:k0 + 16] = t[:, k0 + 8:k0 + 16].copy(), t[:, k0:k0 + 8].copy()
    return _with_factors(case, t, up, with_bias), np.arange(case.shape[0])


def fault_t_row_32_down(case: Case, block: int, with_bias: bool):
    """The rows of one 32-row block paired with the t rows 32 further down (the second chunk's row map off by one block)."""
    t, up = _factors_f64(case)
    m = case.shape[0]
    rows = np.arange(block * 32, min(m, block * 32 + 32))
    rows = rows[rows + 32 < m]
    t[rows] = t[rows + 32]
    return _with_factors(case, t, up, with_bias), rows


def fault_up_row_4_on(case: Case, with_bias: bool):
    """Output channel n finished with svd_up row n + 4 (the other lane group's channels)."""
    t, up = _factors_f64(case)
    n = case.shape[1]
    return _with_factors(case, t, up[np.minimum(np.arange(n) + 4, n - 1)], with_bias), np.arange(case.shape[0])


def fault_down_lost_last_chunk(ex: X.Exact, fmt: str):
    """lowrank_down without the last 16-byte K chunk of svd_down: (t, rows touched)."""
    ce = X.chunk_elems(fmt)
    ints = X.expected_int(ex.ia, ex.ib) - X.int_matmul(ex.ia[:, -ce:], ex.ib[:, -ce:])
    return round_to(ex.acc(ints), fmt), np.nonzero(ex.ia[:, -ce:].any(1))[0]
