"""Operands whose floating-point dot products cannot depend on the order of the additions.

Every entry is i * 2^e with a small integer i and ONE exponent e per row, so every product of output (m, n) is an integer multiple
of 2^(ea[m] + eb[n]) and so is every partial sum: as long as the largest partial sum stays within the adder's span, float32 (and the
matrix core's internal adder) holds all of them exactly, whatever the tile schedule, the K split or the MFMA shape.  The CPU oracle
accumulates in double, which is exact too, so it is the bit-exact expected value of the fp8 / bf16 / f16 GEMMs on these inputs --
the same guarantee the int8 GEMM has on any input.

The span the matrix cores keep was measured, not assumed: tools/micro/mfma_sum_probe.hip, output in profiles/mfma_sum_probe.txt
(C = 2^s plus products equal to 1 is exact up to s = 23 for v_mfma_scale_f32_32x32x64_f8f6f4, v_mfma_f32_32x32x16_bf16 and
v_mfma_f32_32x32x16_f16, and for v_mfma_f32_16x16x32_bf16 / _f16 of sdnq_hip_lowrank_down: the full float32 significand).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

# profiles/mfma_sum_probe.txt: "measured span, accumulator against products (a, b)", one per instruction
# ("bf16" / "f16": v_mfma_f32_32x32x16 of the GEMMs; "*_16x16x32": v_mfma_f32_16x16x32 of sdnq_hip_lowrank_down, the same 23 bits)
MEASURED_SPAN_BITS = {"fp8": 23, "bf16": 23, "f16": 23, "bf16_16x16x32": 23, "f16_16x16x32": 23}
# the budget of the dense cases: the measured span minus 2 bits (alignment cases the probe's few patterns may miss), at most 20
B = {fmt: min(span - 2, 20) for fmt, span in MEASURED_SPAN_BITS.items()}

TORCH_DT = {"fp8": torch.float8_e4m3fn, "bf16": torch.bfloat16, "f16": torch.float16}
TAG_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# row exponents: e4m3 down to its subnormals (multiples of 2^-9) and up to 4 * 2^6 = 256; the 16-bit windows are as wide (bf16) or
# keep |i| 2^e normal and the float16 OUTPUTS of a float16 GEMM finite (f16: products <= 16 * 2^-2)
E_WINDOW = {"fp8": (-9, 6), "bf16": (-8, 7), "f16": (-8, -1)}
IMAX = 4

# the ragged shapes of tests/test_gemm_configs.py::test_every_tile_configuration_bit_exact_vs_oracle plus two small-K ones
RAGGED_SHAPES = ((300, 392, 528), (513, 1288, 208), (64, 64, 64), (1031, 264, 1296), (300, 392, 512), (1031, 520, 1280), (257, 264, 128),
                 (100, 136, 208), (33, 72, 16))
# model size: these reach LD_HT, LD_8P, LD_OG, the tall tile and 128 x 128 under the default heuristics
MODEL_SHAPES = ((1024, 3840, 1280), (1024, 10240, 1280), (4096, 5120, 640), (512, 9216, 3072), (4096, 3072, 3072))
# the shapes of the fused dequantize GEMM test (tests/test_gemm_configs.py), minus its 4096-row one
W8A16_SHAPES = ((200, 392, 528), (1031, 1288, 1296), (33, 64, 64))
# further shapes of the 16-bit GPU tests: K that is no multiple of 16 / of a stage, and a long K
FLOAT_EXTRA_SHAPES = ((100, 136, 200), (100, 136, 208), (64, 128, 4104))


def density_for(k: int) -> float:
    """Short rows need denser operands for every output to sum at least K / 32 nonzero products."""
    return 1.0 if k < 64 else (0.75 if k < 256 else 0.5)


def one_hot_shifts(k: int):
    return sorted({s % k for s in (0, 15, 16, 63, 64, k - 16, k - 1)})


def int_matmul(ia: np.ndarray, ib: np.ndarray) -> np.ndarray:
    """ia [m,k] @ ib [n,k]^T in int64.  The products go through the float64 BLAS (numpy's int64 matmul is a scalar loop), which is exact
    while every sum of magnitudes stays below 2^53: checked."""
    bound = float(np.abs(ia).max(initial=0)) * float(np.abs(ib).max(initial=0)) * ia.shape[1]
    assert bound < 2.0 ** 53, "integer matmul would leave the exact range of float64"
    return np.rint(ia.astype(np.float64) @ ib.astype(np.float64).T).astype(np.int64)


def expected_int(ia: np.ndarray, ib: np.ndarray) -> np.ndarray:
    """The integer sums sum_k ia[m,k] ib[n,k] in int64: the accumulator of output (m, n) in units of 2^(ea[m] + eb[n])."""
    return int_matmul(ia, ib)


def span_bits_of(ia: np.ndarray, ib: np.ndarray, exact: bool = True) -> int:
    """ceil(log2) of the largest sum_k |a b| over all outputs, in units of 2^(ea[m] + eb[n]) -- the smallest product an output can hold
    (an output whose smallest nonzero |ia ib| is larger spans less: this is the conservative reading).  Every partial sum of every
    summation order is bounded by it.  exact=False gives the upper bound max_m sum_k |ia| * max |ib| (and the same with the operands
    swapped) without the m x n x k product, for model-size operands."""
    if exact:
        top = int(int_matmul(np.abs(ia), np.abs(ib)).max(initial=0))
    else:
        top = min(int(np.abs(ia).sum(1).max()) * int(np.abs(ib).max()), int(np.abs(ib).sum(1).max()) * int(np.abs(ia).max()))
    return 0 if top <= 1 else math.ceil(math.log2(top))


@dataclass
class Exact:
    a: torch.Tensor        # [m, k] in the target dtype
    b: torch.Tensor        # [n, k]
    span_bits: int
    ia: np.ndarray         # int64 [m, k]: a = ia * 2^ea[:, None]
    ib: np.ndarray
    ea: np.ndarray         # int64 [m]
    eb: np.ndarray
    fmt: str

    def acc(self, ints=None) -> np.ndarray:
        """The exact accumulators as float64 (integers below 2^53 times a power of two)."""
        ints = expected_int(self.ia, self.ib) if ints is None else ints
        return ints.astype(np.float64) * np.exp2((self.ea[:, None] + self.eb[None, :]).astype(np.float64))

    def codes(self):
        """The operands as the oracle takes them: e4m3 codes (uint8) for fp8, float32 values for the 16-bit formats."""
        if self.fmt == "fp8":
            return self.a.view(torch.uint8).numpy(), self.b.view(torch.uint8).numpy()
        return self.a.float().numpy(), self.b.float().numpy()


def to_format(ints: np.ndarray, e: np.ndarray, fmt: str) -> torch.Tensor:
    vals = ints.astype(np.float64) * np.exp2(e.astype(np.float64))[:, None]
    return torch.from_numpy(vals.astype(np.float32)).to(TORCH_DT[fmt])


def _draw(rng, rows, k, density):
    mag = rng.integers(1, IMAX + 1, size=(rows, k))
    sign = rng.integers(0, 2, size=(rows, k)) * 2 - 1
    keep = rng.random((rows, k)) < density
    return (mag * sign * keep).astype(np.int64)


def exact_operands(m: int, n: int, k: int, seed: int, fmt: str, density=None, e_window=None, exact_span=None) -> Exact:
    """A [m,k], B [n,k] of i * 2^e, i in {0, +-1 .. +-4} (nonzero with probability `density`), e one exponent per row.  Draws again
    (up to 8 times) until at least a quarter of each operand is nonzero, every output sums at least K / 32 nonzero products and
    span_bits <= B[fmt]; raises if no draw does.  Nothing is clipped."""
    density = density_for(k) if density is None else density
    lo, hi = E_WINDOW[fmt] if e_window is None else e_window
    exact_span = (m * n * k <= 2_000_000_000) if exact_span is None else exact_span
    rng = np.random.default_rng(seed)
    why = ""
    for _ in range(8):
        ia, ib = _draw(rng, m, k, density), _draw(rng, n, k, density)
        ea, eb = rng.integers(lo, hi + 1, size=m), rng.integers(lo, hi + 1, size=n)
        if min((ia != 0).mean(), (ib != 0).mean()) < 0.25:
            why = "less than a quarter of an operand is nonzero"
            continue
        if exact_span and int(int_matmul((ia != 0).astype(np.int64), (ib != 0).astype(np.int64)).min()) * 32 < k:
            why = "an output sums fewer than K / 32 nonzero products"
            continue
        span = span_bits_of(ia, ib, exact_span)
        if span > B[fmt]:
            why = f"span of {span} bits exceeds the budget of {B[fmt]}"
            continue
        return Exact(to_format(ia, ea, fmt), to_format(ib, eb, fmt), span, ia, ib, ea, eb, fmt)
    raise ValueError(f"exact_operands({m}, {n}, {k}, seed={seed}, {fmt}, density={density}): {why}")


def exact_bias(ex: Exact, seed: int) -> np.ndarray:
    """A per-channel bias j * 2^(eb[n] + max(ea)), j in {0, +-1 .. +-4}: an integer in the units of EVERY output of its column, so
    accumulator + bias is exact in float32 too (the float GEMMs add the bias before their one rounding).  float32 values that bf16
    and f16 hold."""
    rng = np.random.default_rng(seed)
    j = rng.integers(-IMAX, IMAX + 1, size=ex.eb.shape[0])
    top = int(np.abs(expected_int(np.abs(ex.ia), np.abs(ex.ib))).max()) + IMAX * 2 ** int(ex.ea.max() - ex.ea.min())
    assert top < 2 ** 24, "accumulator + bias would leave the float32 significand"
    return (j * np.exp2((ex.eb + ex.ea.max()).astype(np.float64))).astype(np.float32)


@dataclass
class OneHot:
    a: torch.Tensor
    b: torch.Tensor
    cols: np.ndarray       # the column of row r's only nonzero
    fmt: str

    def acc(self) -> np.ndarray:
        """Each output is ONE product: exact in float32 (and in float64) whatever the adder does."""
        a, b = self.a.float().numpy().astype(np.float64), self.b.float().numpy().astype(np.float64)
        rows = np.arange(a.shape[0])
        return a[rows, self.cols][:, None] * b[:, self.cols].T + 0.0

    codes = Exact.codes


def _arbitrary(rng, shape, fmt) -> torch.Tensor:
    if fmt == "fp8":
        c = rng.integers(0, 256, size=shape).astype(np.uint8)
        c[(c & 0x7f) == 0x7f] = 0x38  # the two NaN codes
        return torch.from_numpy(c).view(torch.float8_e4m3fn)
    return torch.from_numpy((rng.standard_normal(shape) * np.exp2(rng.integers(-6, 4, size=shape))).astype(np.float32)).to(TORCH_DT[fmt])


def one_hot_operands(m: int, n: int, k: int, shift: int, fmt: str = "fp8", seed: int = 0, p: int = 3) -> OneHot:
    """A has exactly one nonzero per row, at column (row * p + shift) mod K with p odd; B is dense with arbitrary finite values of the
    format (every e4m3 code but NaN, subnormals and both zeros included).  No budget applies."""
    assert p % 2 == 1
    rng = np.random.default_rng(seed * 1000003 + shift)
    cols = (np.arange(m) * p + shift) % k
    full = _arbitrary(rng, (m, k), fmt)
    raw = full.view(torch.uint8 if fmt == "fp8" else torch.int16)
    if fmt == "fp8":
        raw[(raw & 0x7f) == 0] = 0x38
    else:
        raw[(raw & 0x7fff) == 0] = 0x3f80 if fmt == "bf16" else 0x3c00
    keep = torch.zeros((m, k), dtype=torch.bool)
    keep[torch.arange(m), torch.from_numpy(cols)] = True
    raw[~keep] = 0
    return OneHot(full, _arbitrary(rng, (n, k), fmt), cols, fmt)


def _fma_f32(v: np.ndarray, s: np.ndarray, c: np.ndarray) -> np.ndarray:
    """float32 fma(v, s, c), one rounding: the product of two float32 is exact in float64; the sum is rounded to ODD in float64 (TwoSum
    gives the residual), which makes the second rounding to float32 the correct single one (53 >= 2 * 24 + 2)."""
    p = v.astype(np.float64) * s.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    t = p + c
    cc = t - p
    err = (p - (t - cc)) + (c - cc)
    fix = (err != 0) & ((t.view(np.int64) & 1) == 0)
    t = np.where(fix, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(np.float32)


def epilogue(acc: np.ndarray, sa: np.ndarray, sb: np.ndarray, bias, tag: str) -> np.ndarray:
    """The scaled matmul's epilogue on exact accumulators, independent of the C oracle: cast(fma(f32(acc) * sa, sb, bias)), or
    cast((f32(acc) * sa) * sb) without bias; bias None | [N] | [M,N] float32.  Returns float32 holding `tag` values."""
    f = np.float32
    a32 = acc.astype(f)
    assert np.array_equal(a32.astype(np.float64), acc), "accumulators must be float32 values"
    v = a32 * np.asarray(sa, dtype=f).reshape(-1, 1)
    sbv = np.asarray(sb, dtype=f).reshape(1, -1)
    if bias is None:
        r = v * sbv
    else:
        bias = np.asarray(bias, dtype=f)
        r = _fma_f32(v, sbv, bias.reshape(1, -1) if bias.ndim == 1 else bias)
    return torch.from_numpy(np.ascontiguousarray(r)).to(TAG_DT[tag]).float().numpy()


def chunk_elems(fmt: str) -> int:
    """Elements in one 16-byte K chunk (the unit of the LDS-DMA, the swizzle and an fp8 lane's two fragment reads)."""
    return 16 if fmt == "fp8" else 8


def corrupt_drop(ex: Exact, kk: int):
    """A kernel that loses K element kk: (integer accumulators, rows it touches)."""
    return expected_int(ex.ia, ex.ib) - ex.ia[:, kk:kk + 1] * ex.ib[:, kk][None, :], np.nonzero(ex.ia[:, kk])[0]


def corrupt_swap_b_chunks(ex: Exact, c0: int, c1: int):
    """A kernel that reads two 16-byte K chunks of B (only) in each other's place."""
    ce = chunk_elems(ex.fmt)
    ib = ex.ib.copy()
    ib[:, c0 * ce:(c0 + 1) * ce], ib[:, c1 * ce:(c1 + 1) * ce] = ex.ib[:, c1 * ce:(c1 + 1) * ce], ex.ib[:, c0 * ce:(c0 + 1) * ce]
    touched = np.nonzero((ex.ia[:, c0 * ce:(c0 + 1) * ce] != ex.ia[:, c1 * ce:(c1 + 1) * ce]).any(1))[0]
    return expected_int(ex.ia, ib), touched


def corrupt_double_tail(ex: Exact):
    """A kernel that counts the last 16-byte chunk of K twice."""
    ce = chunk_elems(ex.fmt)
    return expected_int(ex.ia, ex.ib) + int_matmul(ex.ia[:, -ce:], ex.ib[:, -ce:]), np.nonzero(ex.ia[:, -ce:].any(1))[0]
