"""Inputs and CPU expected values of the DoRA kernels' tests (tests/test_dora_exact_gpu.py, tests/test_dora_gpu.py, tests/test_dora_host.py):
sdnq_hip_dora_normsq(_dense), sdnq_hip_lowrank_add_dora and sdnq_hip_dora_bwd restated in numpy, in float64 and in float32-exact forms.

    normsq   out[n] = sum_k e^2,  e = fma_f32(scale, acc[n][k], w32[n][k])       acc = up . down, exact in float32 in every order
    add      y = round_dtype( fma_f32(c * scale, acc, inner) ),  inner = z if c == 1 else fma_f32(c - 1, z - b, z)
             (acc == 0: y = round_dtype(inner)); c * scale, c - 1 and z - b one float32 operation each
    bwd      g = round_dtype( f32(dy) * c ),  q[n] = sum_i f32(dy[i][n]) * (f32(y[i][n]) - f32(b[n]))

The exact cases keep every value an integer multiple of ONE quantum per output (row n of the norm, column n of q) and the sum of the
magnitudes below 2^24 quanta, so every partial sum of every summation order is a float32 value: `assert_exact` checks it on the CPU, from
the float64 restatement, before anything is compared.
"""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

from oracle import oracle as O
from tests import exact_inputs as X

DB_SLAB = 256   # rows per partial sum of sdnq_hip_dora_bwd: DB_SLAB of csrc/dora.hip (test_dora_host.py compares the two)
DN_KC = 256     # columns per workgroup iteration of the norm kernel: DN_KC of csrc/dora.hip
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SCALE = 0.5


def constants_in_source() -> dict:
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sdnq_amd", "csrc", "dora.hip")
    with open(src) as f:
        text = f.read()
    return {name: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("DB_SLAB", "DN_KC")}


def round_f32_to(a32: np.ndarray, tag: str) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(DT[tag]).float().numpy()


def assert_exact(terms: np.ndarray, quantum: np.ndarray, axis: int) -> None:
    """Every term (float64) is an integer number of quanta and the magnitudes along `axis` sum to less than 2^24 of them: every partial
    sum in every order is an integer below 2^24 in units of the quantum, a float32 value."""
    t = terms / quantum
    assert np.array_equal(t, np.rint(t)), "a term is not an integer number of quanta"
    assert float(np.abs(t).sum(axis).max(initial=0.0)) < 2.0 ** 24, "a sum would leave the float32 significand"


# ---- the norm ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Fmt:
    """One storage-format bucket of the dequantizer: weights_dtype, group size (0: one scale per row), the dtype of scale / zero point,
    codebook."""
    wdt: str
    group: int = 0
    scale_tag: str = "f32"
    codebook: bool = False

    @property
    def id(self) -> str:
        return f"{self.wdt}-g{self.group}-{self.scale_tag}" + ("-codebook" if self.codebook else "")


FORMATS = (Fmt("int8"), Fmt("uint4", 32), Fmt("uint4", 64), Fmt("uint3", 16), Fmt("int5", 16), Fmt("float8_e4m3fn"), Fmt("float6_e3m2fn", 16),
           Fmt("uint4", 16, codebook=True), Fmt("int8", 0, "bf16"), Fmt("uint4", 16, "f16"), Fmt("uint8", 16))
ZERO_POINT_FORMATS = tuple(f.id for f in FORMATS if f.wdt.startswith("uint") and not f.codebook)


def _store(codes: np.ndarray, wdt: str) -> np.ndarray:
    bits = O.dtype_info(wdt)["bits"]
    return codes.astype(np.uint8).reshape(-1) if bits == 8 else O.pack_codes(codes, bits)


@functools.lru_cache(maxsize=None)
def _code_values(wdt: str) -> np.ndarray:
    """The value of every code before the scale, read back through the oracle's weight_values."""
    bits = O.dtype_info(wdt)["bits"]
    codes = np.resize(np.arange(1 << bits), max(16, 1 << bits))
    return O.weight_values(_store(codes, wdt), wdt, (codes.size,)).astype(np.float64)[:1 << bits]


@dataclass
class Weight:
    fmt: Fmt
    n: int
    k: int
    stored: np.ndarray     # the bytes the layer stores
    scale: np.ndarray      # float64 [n, G] (codebook: the level table [n, G, L])
    zp: np.ndarray | None  # float64 [n, G]
    w: np.ndarray          # float64 [n, k]: the dequantized weight, exact
    er: np.ndarray         # int64 [n]: the row's exponent; every w[n] is an integer multiple of 2^er[n]

    def device(self, device):
        from sdnq_amd import ops
        sdt = DT[self.fmt.scale_tag]
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(sdt).to(device)  # noqa: E731
        return ops.make_quant_weight(self.fmt.wdt, torch.from_numpy(self.stored).to(device), t(self.scale), t(self.zp), None, None, self.n,
                                     self.k, self.fmt.group or self.k, transposed=False, codebook=self.fmt.codebook)


def plant_weight(fmt: Fmt, n: int, k: int, seed: int) -> Weight:
    """Codes whose values are small integers (|v| <= 4; a codebook's levels |v| <= 8), scales 2^(er[n] + eg[n][g]) with eg in {0, 1}, the
    zero point of an unsigned format -2^(bits - 1) scale: w[n][k] is an integer of magnitude <= 16 times 2^er[n]."""
    rng = np.random.default_rng(seed)
    info = O.dtype_info(fmt.wdt)
    bits, group = info["bits"], fmt.group or k
    assert k % group == 0
    g = k // group
    er = rng.integers(-3, 4, size=n)
    s = np.exp2((er[:, None] + rng.integers(0, 2, size=(n, g))).astype(np.float64))
    vals = _code_values(fmt.wdt)
    zp = None
    if fmt.codebook:
        levels = 1 << bits
        perm = ((np.arange(levels) * 5) % levels - levels // 2).astype(np.float64)
        codes = rng.integers(0, levels, size=(n, k))
        table = perm[None, None, :] * s[:, :, None]
        w = table[np.arange(n)[:, None], np.arange(k)[None, :] // group, codes]
        scale = table
    else:
        off = float(1 << (bits - 1)) if info["kind"] == "uint" else 0.0
        eff = vals - off
        want = np.arange(-4, 5, dtype=np.float64)
        allowed = np.array([int(np.nonzero(eff == v)[0][0]) for v in want if (eff == v).any()])
        assert allowed.size >= 5, f"{fmt.wdt}: too few codes with small integer values"
        codes = allowed[rng.integers(0, allowed.size, size=(n, k))]
        sk = np.repeat(s, group, axis=1)
        w = eff[codes] * sk
        scale = s
        if info["kind"] == "uint":
            zp = -off * s
    return Weight(fmt, n, k, _store(codes.reshape(-1), fmt.wdt), scale, zp, w, er)


def plant_factors(n: int, k: int, rank: int, er: np.ndarray, seed: int):
    """(up [n, rank], down [rank, k]) as float64: up dense, integers in {+-1, +-2} times 2^er[n]; every column of down has at most four
    entries +-1, at random ranks -- so |acc| <= 8 * 2^er[n] while every rank column takes part in some output."""
    rng = np.random.default_rng(seed)
    up = rng.integers(1, 3, size=(n, rank)) * (rng.integers(0, 2, size=(n, rank)) * 2 - 1) * np.exp2(er.astype(np.float64))[:, None]
    down = np.zeros((rank, k))
    for _ in range(4):
        down[rng.integers(0, rank, size=k), np.arange(k)] = rng.integers(0, 2, size=k) * 2 - 1
    return up, down


def normsq_f64(w: np.ndarray, up, down, scale: float):
    """(normsq [n], e [n, k]) in float64."""
    e = w if up is None else w + scale * (up @ down)
    return (e * e).sum(1), e


def normsq_expected(w: np.ndarray, up, down, scale: float, er: np.ndarray) -> np.ndarray:
    """The float32 result on exact-sum operands, with the exactness asserted: e is an integer number of half quanta 2^(er - 1), the
    squares of quanta 2^(2 er - 2)."""
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w), "the weight must hold float32 values"
    out, e = normsq_f64(w, up, down, scale)
    if up is not None:
        acc = up @ down
        # the rank sum: integer entries of up (in units of 2^er) times integer entries of down, the magnitudes summing below 2^24
        assert_exact(up, np.exp2(er.astype(np.float64))[:, None], 1)
        assert np.array_equal(down, np.rint(down))
        assert float(((np.abs(up) @ np.abs(down)) / np.exp2(er.astype(np.float64))[:, None]).max()) < 2.0 ** 24
        assert np.array_equal(X._fma_f32(acc.astype(np.float32), np.full(acc.shape, scale, dtype=np.float32), w32).astype(np.float64), e)
    assert_exact(e, np.exp2(er.astype(np.float64) - 1)[:, None], 1)
    assert_exact(e * e, np.exp2(2.0 * er - 2)[:, None], 1)
    return out.astype(np.float32)


# ---- the add's epilogue --------------------------------------------------------------------------------------------------------------------
def add_dora_expected(acc: np.ndarray, z: np.ndarray, c: np.ndarray, bias, scale: float, tag: str) -> np.ndarray:
    """acc [m, n] float64 holding float32 values, z [m, n] float32 holding `tag` values, c [n] float32, bias [n] float32 holding `tag`
    values or None: the stored y as float32, in the operation order of the kernel."""
    f = np.float32
    a32 = acc.astype(f)
    assert np.array_equal(a32.astype(np.float64), acc), "accumulators must be float32 values"
    z = z.astype(f)
    cb = np.broadcast_to(c.astype(f)[None, :], z.shape)
    b = np.zeros(z.shape, dtype=f) if bias is None else np.broadcast_to(bias.astype(f)[None, :], z.shape)
    cm1 = cb - f(1.0)
    cs = cb * f(scale)
    inner = np.where(cm1 == 0, z, X._fma_f32(cm1, z - b, z))
    return round_f32_to(np.where(a32 == 0, inner, X._fma_f32(cs, a32, inner)), tag)


# ---- the backward pass ---------------------------------------------------------------------------------------------------------------------
def bwd_g_expected(dy: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    return (dy.float() * c.float()[None, :]).to(dy.dtype)


def bwd_case(m: int, n: int, tag: str, seed: int, with_bias: bool = True):
    """(dy, y, bias | None in the dtype, q expected float32): dy small integers, y and bias integers times 2^en[n] -- every product an
    integer in units of 2^en[n], the exactness of the column sums asserted."""
    rng = np.random.default_rng(seed)
    en = rng.integers(-4, 4, size=n)
    unit = np.exp2(en.astype(np.float64))
    dy = rng.integers(-4, 5, size=(m, n)).astype(np.float64)
    y = rng.integers(-4, 5, size=(m, n)) * unit[None, :]
    b = rng.integers(-4, 5, size=n) * unit if with_bias else np.zeros(n)
    terms = dy * (y - b[None, :])
    assert_exact(y - b[None, :], unit[None, :], 0)
    assert_exact(terms, unit[None, :], 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[tag])  # noqa: E731
    return t(dy), t(y), (t(b) if with_bias else None), terms.sum(0).astype(np.float32)
