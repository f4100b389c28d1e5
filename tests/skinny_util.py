"""Planted weights, exact activations and the case table of the few-row linear kernels (sdnq_amd/csrc/skinny.hip).

Every case is built so that nothing the kernel computes can round before the ONE rounding of the output: the stored codes, scales, zero
points and SVD factors are chosen (not quantized from a float weight), the weight element the kernel forms -- v s | v s + z, plus the rank
product, un-rotated on Hadamard layers -- is a value of the activation dtype T, and every product x w of output (m, n) is an integer multiple
of one power of two with sum_k |x w| below 2^20 of it.  Then every partial sum of every order is exact in float32: the fmaf chain, the packed
dot products, the wave reduction and the `red` reduction all hold the same numbers, and the expected output is round_T(float64 sum + bias).
The conditions are asserted here on the CPU for every case (`plant`), they are not measurements of the kernel.

`launch_path` restates the launcher's rule (skinny.hip: sdnq_hip_linear_skinny, sdnq_hip_linear_skinny_svd), `CASES` is laid out so that every
path meets every K class of its kernel's loop.  Shared by tests/test_skinny_host.py (CPU) and tests/test_skinny_census_gpu.py.
"""
import functools
import math
import os
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import oracle as O
from tests import exact_inputs as X

TAG_DT = X.TAG_DT
BUDGET_BITS = X.B["bf16"]  # 20: the budget of the GEMM exact-sum tests, below the measured 23-bit span
N_PLAIN, N_SVD = 70, 72    # 70: the last workgroup's tail waves return; 72: the last 32-channel workgroup is clamped to N - 1
PERIOD = {"generic": 1024, "fast": 4096, "had256": 4096, "svd": 128, "svd32": 128}   # columns per trip of the kernel's K loop
BLOCK = {"generic": 1024, "fast": 1024, "had256": 256, "svd": 32, "svd32": 32}       # pass / chunk / 256-group / 32-block inside a trip
ALL_PATHS = tuple([f"generic-MR{r}" for r in (1, 2, 4, 8)] +
                  [f"{k}-{b}bit-MR{r}" for k in ("fast", "had256", "svd", "svd32") for b in (8, 4) for r in (1, 2, 4)])


def require_default_tuning():
    """The case table is laid out for the launcher's own rule: with the Hadamard switch set the cases would run on other kernels than they claim."""
    assert "SDNQ_HIP_HADAMARD_MFMA" not in os.environ, "unset SDNQ_HIP_HADAMARD_MFMA: the few-row census needs the launcher's own choice of kernel"


def _int_bits(wdt: str, codebook: bool) -> int:
    """int_code_bits (weight_dev.h): 8 for raw 8-bit integers, 4 for packed 4-bit integers, 0 for anything else."""
    info = O.dtype_info(wdt)
    if codebook or info["kind"] not in ("int", "uint"):
        return 0
    return info["bits"] if info["bits"] in (8, 4) else 0


def launch_path(wdt, group_size, scale_tag, had, tag, m, k, rank=0, ldx=None, x_align=16, codebook=False) -> str:
    """The kernel and template cell the launcher picks: generic-MR{1,2,4,8} | fast-{8,4}bit-MR{1,2,4} | had256-.. | svd-.. | svd32-..
    (group_size is the layer's: <= 0 means one group per row; x_align: the largest power of two <= 16 dividing x's address)."""
    require_default_tuning()
    ldx = k if ldx is None else ldx
    gs = group_size if group_size > 0 else k
    assert k % 16 == 0 and k % gs == 0 and ldx >= k, "fill_params"
    g_count = k // gs
    bits = _int_bits(wdt, codebook)
    eb = 4 if tag == "f32" else 2
    if rank:  # sdnq_hip_linear_skinny_svd
        assert tag in ("bf16", "f16") and scale_tag in ("f32", tag) and bits and gs % 4 == 0
        assert 0 < m <= 4 and k % 32 == 0 and rank % 16 == 0
        rows = 1 if m <= 1 else (2 if m <= 2 else 4)
        lds = rows * k * 4
        assert lds <= 150 * 1024
        lds32 = lds // 2 + 4 * 4 * 3072 + 32 * g_count * 8
        rank32 = (rank == 32 and lds32 <= 150 * 1024 and gs % 16 == 0 and g_count <= 64 and (bits == 8 or k % 64 == 0)
                  and x_align % 16 == 0 and (ldx * 2) % 16 == 0)
        return f"{'svd32' if rank32 else 'svd'}-{bits}bit-MR{rows}"
    assert 0 < m <= 64 and x_align % 16 == 0 and (ldx * eb) % 16 == 0
    assert had == 0 or (4 <= had <= 512 and had & (had - 1) == 0 and k % had == 0)
    tuned = bool(bits) and m <= 4 and scale_tag in ("f32", tag)
    rows_tuned = 1 if m == 1 else (2 if m == 2 else 4)
    if tuned and had == 256 and tag != "f32" and gs % 4 == 0:
        return f"had256-{bits}bit-MR{rows_tuned}"
    if tuned and gs % 16 == 0:
        return f"fast-{bits}bit-MR{rows_tuned}"
    return f"generic-MR{1 if m == 1 else (2 if m <= 2 else (4 if m <= 4 else 8))}"


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kernel: str            # the kernel the case is laid out for; `path` says where the launcher sends it
    wdt: str
    gs: int                # 0: one group per row
    tag: str
    m: int
    k: int
    had: int = 0
    rank: int = 0
    scale_tag: str = "f32"
    codebook: bool = False
    strided: bool = False  # x = wide[:, :K] with 64 extra columns
    bias: bool = True
    x_align: int = 16      # 8: x starts 8 bytes past a 16-byte boundary
    repeat: int = 1
    note: str = ""

    @property
    def n(self) -> int:
        return N_SVD if self.rank else N_PLAIN

    @property
    def group(self) -> int:
        return self.gs if self.gs > 0 else self.k

    @property
    def ldx(self) -> int:
        return self.k + 64 if self.strided else self.k

    @property
    def path(self) -> str:
        return launch_path(self.wdt, self.gs, self.scale_tag, self.had, self.tag, self.m, self.k, self.rank, self.ldx, self.x_align, self.codebook)

    @property
    def id(self) -> str:
        opts = [f"had{self.had}" if self.had else "", f"r{self.rank}" if self.rank else "", f"s{self.scale_tag}" if self.scale_tag != "f32" else "",
                "cb" if self.codebook else "", "strided" if self.strided else "", "" if self.bias else "nobias",
                f"a{self.x_align}" if self.x_align != 16 else "", f"x{self.repeat}" if self.repeat > 1 else ""]
        return "-".join([self.kernel, self.wdt, f"g{self.gs}", self.tag, f"m{self.m}", f"k{self.k}"] + [o for o in opts if o])


K_CLASSES = {
    "generic": (1008, 1024, 1040, 2064),     # dead lanes in one pass | one full pass | a second pass with one live lane | three passes
    "fast": (1040, 4096, 4112, 5136),        # second chunk | one full stretch | second stretch: one live lane, three dead chunks | two chunks there
    "had256": (256, 3840, 4096, 4352),       # one group | 15 of 16 | a full pass | a second pass with one group
    "svd": (32, 128, 160, 672),              # three idle waves | one block per wave | a second trip for wave 0 | six trips, the last for wave 0 alone
    "svd32-8": (32, 96, 512, 544, 640, 1056),  # 512: four ring slots, none refilled; 544 / 640: slot 0 read again after its refill; 1056: ragged
    "svd32-4": (64, 576, 640, 1088),
}
FAST_FORMATS = (("int8", 0), ("uint8", 0), ("int4", 64), ("uint4", 16))  # int4: g = 16 where 64 does not divide K
HAD256_FORMATS = (("int8", 0), ("uint8", 0), ("int4", 64), ("uint4", 64))


def _table():
    c = []
    # generic: formats the tuned kernels do not take at M <= 4, the tuned formats above
    for k in K_CLASSES["generic"]:
        for tag in ("bf16", "f16", "f32"):
            for i, m in enumerate((1, 2, 3, 5, 8, 9, 32)):
                wdt, gs = (("int5", 0), ("int6", 16))[(i + k // 16) % 2] if m <= 4 else (("int8", 0), ("uint4", 16), ("uint8", 16))[(i + k // 16) % 3]
                c.append(Case("generic", wdt, gs, tag, m, k))
    for k in K_CLASSES["fast"]:
        for tag in ("bf16", "f16", "f32"):
            for wdt, gs in FAST_FORMATS:
                for m in (1, 2, 3, 4):
                    c.append(Case("fast", wdt, gs if k % max(gs, 1) == 0 else 16, tag, m, k))
    for k in K_CLASSES["had256"]:
        for tag in ("bf16", "f16"):
            for wdt, gs in HAD256_FORMATS:
                for m in (1, 2, 3):
                    c.append(Case("had256", wdt, gs, tag, m, k, had=256))
    for k in K_CLASSES["svd"]:
        for tag in ("bf16", "f16"):
            for wdt, gs in (("int8", 0), ("uint8", 0), ("int4", 32), ("uint4", 32)):
                for m in (1, 2, 3):
                    for rank in (16, 48, 32):
                        c.append(Case("svd", wdt, gs, tag, m, k, rank=rank, x_align=8 if rank == 32 else 16))
    for key, fmts in (("svd32-8", (("int8", 0), ("uint8", 0))), ("svd32-4", (("int4", 64), ("uint4", 64)))):
        for k in K_CLASSES[key]:
            for tag in ("bf16", "f16"):
                for wdt, gs in fmts:
                    for m in (1, 2, 4):
                        c.append(Case("svd32", wdt, gs, tag, m, k, rank=32))
    # one of each storage family on the generic kernel (K = 1152: a second pass with 8 live lanes, every group size divides it)
    for i, (wdt, gs, cb) in enumerate((("int3", 32, False), ("int5", 0, False), ("uint7", 128, False), ("uint2", 16, False),
                                       ("float6_e3m2fn", 32, False), ("fp8", 0, False), ("uint4", 64, True))):
        c.append(Case("generic", wdt, gs, ("bf16", "f16", "f32")[i % 3], (3, 1, 2, 5)[i % 4], 1152, codebook=cb, note="storage family"))
    c.append(Case("generic", "int8", 0, "f16", 2, 1040, scale_tag="bf16", note="bf16 scales: the product is rounded to the scale dtype"))
    # the FWHT un-rotation inside the fast and the generic kernel
    c += [Case("fast", "int8", 0, "bf16", 3, 1040, had=16, note="FWHT"), Case("fast", "int4", 64, "f16", 1, 1280, had=64, note="FWHT"),
          Case("fast", "int8", 0, "f32", 2, 1280, had=256, note="FWHT: float32 activations keep group 256 off the matrix cores"),
          Case("fast", "uint4", 16, "bf16", 4, 1040, had=4, note="FWHT")]
    c += [Case("generic", "int8", 0, ("bf16", "f16", "f32")[i], 5, 1280, had=g, note="FWHT") for i, g in enumerate((16, 64, 256))]
    # rank 32 off the DMA kernel, and groups on it
    c += [Case("svd", "int8", 16, "bf16", 2, 1056, rank=32, note="G = 66 > 64: the generic SVD kernel"),
          Case("svd32", "uint4", 32, "bf16", 4, 1088, rank=32, note="per-group scales and zero points, G = 34"),
          Case("svd32", "uint8", 32, "f16", 2, 1056, rank=32, note="per-group scales and zero points, G = 33")]
    # per kernel: strided x, no bias, the same call three times
    for kern, wdt, gs, tag, m, k, kw in (("generic", "int5", 0, "bf16", 9, 2064, {}), ("fast", "int4", 16, "bf16", 4, 5136, {}),
                                         ("had256", "int4", 64, "bf16", 3, 4352, dict(had=256)), ("svd", "int8", 0, "bf16", 3, 672, dict(rank=16)),
                                         ("svd32", "int8", 0, "bf16", 4, 1056, dict(rank=32))):
        c += [Case(kern, wdt, gs, tag, m, k, strided=True, **kw), Case(kern, wdt, gs, tag, m, k, bias=False, **kw),
              Case(kern, wdt, gs, "f16", 1, k, bias=False, **kw), Case(kern, wdt, gs, tag, m, k, repeat=3, **kw)]
    c.append(Case("generic", "int8", 0, "bf16", 32, 1040, bias=False, note="no bias at M = 32"))
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    return tuple(c)


CASES = _table()
BY_ID = {c.id: c for c in CASES}


def cases_of(kernel):
    return [c for c in CASES if c.kernel == kernel]


# ------------------------------------------------------------------------------------------------
# planted data
# ------------------------------------------------------------------------------------------------
def _store(codes: np.ndarray, wdt: str) -> np.ndarray:
    """Unsigned codes (flat, [N][K] order) -> the bytes the layer stores: the oracle's packer, or the raw byte."""
    info = O.dtype_info(wdt)
    if info["bits"] == 8:
        return codes.astype(np.uint8).reshape(-1)
    return O.pack_codes(codes, info["bits"])


@functools.lru_cache(maxsize=None)
def _code_values(wdt: str) -> np.ndarray:
    """value of every code, read back through the oracle's weight_values (pinned to the reference's vectors)."""
    bits = O.dtype_info(wdt)["bits"]
    codes = np.resize(np.arange(1 << bits), max(16, 1 << bits))
    vals = O.weight_values(_store(codes, wdt), wdt, (codes.size,)).astype(np.float64)
    return vals[:1 << bits]


def _effective(case: Case) -> np.ndarray:
    """What code c contributes before the scale: its value, minus 2^(bits-1) for the unsigned formats (z = -2^(bits-1) s), or its level of the
    codebook (a permutation of the signed range, the same for every group up to the group's power of two)."""
    info = O.dtype_info(case.wdt)
    v = _code_values(case.wdt)
    if case.codebook:
        levels = 1 << info["bits"]
        return ((np.arange(levels) * 5) % levels - levels // 2).astype(np.float64)
    if info["kind"] == "uint":
        return v - float(1 << (info["bits"] - 1))
    return v


def _low_exp(a: np.ndarray, axis: int) -> np.ndarray:
    """Exponent of the largest power of two dividing every element along `axis` (elements are multiples of 2^-40 below 2^12)."""
    i = np.rint(np.abs(a) * 2.0 ** 40).astype(np.int64)
    assert np.array_equal(i.astype(np.float64) * 2.0 ** -40, np.abs(a)), "values finer than 2^-40"
    low = np.where(i == 0, np.int64(1) << 62, i & -i).min(axis=axis)
    assert (low < (np.int64(1) << 62)).all(), "an all-zero row"
    return np.log2(low.astype(np.float64)).astype(np.int64) - 40


def representable(a: np.ndarray, tag: str) -> bool:
    a32 = a.astype(np.float32)
    if not np.array_equal(a32.astype(np.float64), a):
        return False
    return bool(np.array_equal(O.round_dtype(a32, tag), a32))


def all_normal(a: np.ndarray, tag: str) -> bool:
    tiny = {"bf16": 2.0 ** -126, "f32": 2.0 ** -126, "f16": 2.0 ** -14}[tag]
    big = {"bf16": 3.0e38, "f32": 3.0e38, "f16": 65504.0}[tag]
    nz = np.abs(a[a != 0])
    return bool(nz.size == 0 or (nz.min() >= tiny and nz.max() <= big))


def round_t(a: np.ndarray, tag: str) -> np.ndarray:
    """float64 -> T, ONE rounding: asserted exact in float32 first (it is, inside the budget)."""
    a32 = a.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a), "a sum left float32: outside the exact budget"
    return O.round_dtype(a32, tag)


@dataclass
class Planted:
    case: Case
    stored: np.ndarray      # uint8 words, [N][K] element order
    scale: np.ndarray       # float32 [N, G] ([N, G, L] for a codebook)
    zp: np.ndarray | None   # float32 [N, G]
    up: np.ndarray | None   # float64 [N, R]
    down: np.ndarray | None  # float64 [R, K]
    w_stored: np.ndarray    # float64 [N, K]: v s | v s + z (+ up down), as dequantized BEFORE the un-rotation
    w: np.ndarray           # float64 [N, K]: the weight element the kernel multiplies with
    x: np.ndarray           # float64 [M, K]
    bias: np.ndarray | None  # float64 [N]
    span_bits: int
    density: float
    rare: float
    ex: np.ndarray = field(default=None)
    ew: np.ndarray = field(default=None)

    def expected(self, w=None, x=None) -> np.ndarray:
        """round_T(float64 sum + bias) as float32 values of T."""
        w = self.w if w is None else w
        x = self.x if x is None else x
        acc = x @ w.T + 0.0
        if self.bias is not None:
            acc = acc + self.bias[None, :]
        return round_t(acc, self.case.tag)


def _rng(case: Case, salt) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(f"{case.id}/{salt}".encode()))


def _pick(rng, eff, shape, rare, small_lim, rare_lim):
    """Codes: small effective values everywhere, any code up to rare_lim at a planted minority."""
    grid = np.abs(eff * 4 - np.rint(eff * 4)) == 0  # multiples of 1/4 (every integer code; the float formats' coarse end)
    small = np.nonzero(grid & (np.abs(eff) <= small_lim))[0]
    wide = np.nonzero(grid & (np.abs(eff) <= rare_lim))[0]
    codes = small[rng.integers(0, small.size, size=shape)]
    pick = rng.random(shape) < rare
    return np.where(pick, wide[rng.integers(0, wide.size, size=shape)], codes)


def _weight(case: Case, rare: float):
    """codes [N, K], scale exponents [N, G], and the float64 weight as dequantized (before SVD and un-rotation)."""
    rng = _rng(case, "w")
    n, k, gs = case.n, case.k, case.group
    g_count = k // gs
    eff = _effective(case)
    bits = O.dtype_info(case.wdt)["bits"]
    is_int = O.dtype_info(case.wdt)["kind"] in ("int", "uint")
    rare_lim = float(1 << (bits - 1)) if is_int else 32.0
    if case.rank:
        e = rng.integers(0, 2, size=(n, g_count))                 # v s + up down stays an integer of magnitude <= 256
    elif case.had:
        e = rng.integers(-3, 0, size=(n, g_count))
    else:
        e = rng.integers(-4, -1, size=(n, g_count))
    ek = np.repeat(e, gs, axis=1)
    if not case.had:
        codes = _pick(rng, eff, (n, k), rare, 2.0, rare_lim)
        if case.rank:  # where s = 2 the full-range codes are halved
            half = _pick(rng, eff, (n, k), rare, 2.0, rare_lim / 2)
            codes = np.where(ek == 1, half, codes)
    else:
        # stored rows of a rotated layer, per Hadamard group: a spike q s e_j (un-rotates to +-q s / sqrt(g) everywhere) or c walsh_j
        # (un-rotates to c sqrt(g) e_j); c = 4 * 2^min(e) is formed in every scale group of the Hadamard group from the code 4 >> (e - min e)
        g = case.had
        code_of = {float(v): i for i, v in enumerate(eff)}
        walsh = np.rint(O.hadamard_matrix(g, "f32").astype(np.float64) * math.sqrt(g))
        effk = np.zeros((n, k))
        for h in range(k // g):
            sl = slice(h * g, (h + 1) * g)
            emin = ek[:, sl].min(axis=1, keepdims=True)
            de = ek[:, sl] - emin
            j = rng.integers(0, g, size=n)
            mag = np.where(de == 0, 4.0, np.where(de == 1, 2.0, 1.0)) * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)
            rows_walsh = walsh[j] * mag
            spike_codes = _pick(rng, eff, (n,), max(rare * 2, 0.0), 4.0, rare_lim)
            q = eff[spike_codes]
            q = np.where(q == 0, 1.0, q)
            rows_spike = np.zeros((n, g))
            rows_spike[np.arange(n), j] = q
            is_walsh = rng.random((n, 1)) < 0.5
            effk[:, sl] = np.where(is_walsh, rows_walsh, rows_spike)
        codes = np.vectorize(code_of.__getitem__, otypes=[np.int64])(effk)
    w = eff[codes] * np.exp2(ek.astype(np.float64))
    return codes, e, w


def _unrotate(w: np.ndarray, g: int) -> np.ndarray:
    h = O.hadamard_matrix(g, "f32").astype(np.float64)  # +-1 / sqrt(g), a power of two for g = 4, 16, 64, 256: exact
    assert g in (4, 16, 64, 256)
    n, k = w.shape
    return (w.reshape(n, k // g, g) @ h).reshape(n, k)


def _svd(case: Case):
    rng = _rng(case, "svd")
    n, k, r = case.n, case.k, case.rank
    up = rng.integers(-3, 4, size=(n, r)) * (rng.random((n, r)) < 0.5)
    down = np.zeros((r, k))
    down[rng.integers(0, r, size=k), np.arange(k)] = rng.integers(1, 3, size=k) * (rng.integers(0, 2, size=k) * 2 - 1)
    return up.astype(np.float64), down


@functools.lru_cache(maxsize=64)  # a case holds up to 3 MB; the census reuses the largest cases of the exact-sum test
def plant(case: Case) -> Planted:
    """The case's planted weight, activations and bias, inside the exact budget: the full-range codes and then x are thinned until the span fits
    (the budget is never raised).  Asserts every condition the exactness argument needs."""
    tag = case.tag
    last = None
    for density, rare in ((0.5, 1 / 16), (0.5, 1 / 64), (0.25, 1 / 64), (0.125, 1 / 128), (0.0625, 1 / 256)):
        codes, e, w_deq = _weight(case, rare)
        up = down = None
        w_stored = w_deq
        if case.rank:
            up, down = _svd(case)
            assert representable(w_deq, tag), (case.id, "round_T(v s) is not exact")
            w_stored = w_deq + up @ down
            assert np.abs(w_stored).max() <= 256 and np.array_equal(w_stored, np.rint(w_stored)), (case.id, "v s + up down must be an integer <= 256")
        w = _unrotate(w_stored, case.had) if case.had else w_stored
        rng = _rng(case, "x")
        ix = X._draw(rng, case.m, case.k, density)
        ix[:, -1] = np.where(ix[:, -1] == 0, 1, ix[:, -1])  # the last column is always live
        ix[:, SWAP_A], ix[:, case.k - TAIL_B] = 4, -3           # the pair edit_swap_columns exchanges: live and different in every row
        ea = rng.integers(-6, -2, size=case.m)
        x = ix.astype(np.float64) * np.exp2(ea.astype(np.float64))[:, None]
        ew, ex = _low_exp(w, 1), _low_exp(x, 1)
        bias = None
        if case.bias:
            bias = rng.integers(-X.IMAX, X.IMAX + 1, size=case.n) * np.exp2((ew + ex.max()).astype(np.float64))
        top = np.abs(x) @ np.abs(w).T + (0.0 if bias is None else np.abs(bias)[None, :])
        units = top / np.exp2((ex[:, None] + ew[None, :]).astype(np.float64))
        span = math.ceil(math.log2(max(float(units.max()), 1.0)))
        last = (span, density, rare)
        if span <= BUDGET_BITS:
            break
    else:
        raise AssertionError(f"{case.id}: span {last[0]} bits at density {last[1]}, rare {last[2]}: over the budget of {BUDGET_BITS}")
    info = O.dtype_info(case.wdt)
    gs, g_count = case.group, case.k // case.group
    scale = np.exp2(e.astype(np.float64)).astype(np.float32)
    zp = None
    if case.codebook:
        scale = (_effective(case)[None, None, :] * np.exp2(e.astype(np.float64))[:, :, None]).astype(np.float32)
    elif info["kind"] == "uint":
        zp = (-float(1 << (info["bits"] - 1)) * scale).astype(np.float32)
    stored = _store(codes.reshape(-1), case.wdt)
    p = Planted(case, stored, scale, zp, up, down, w_stored, w, x, bias, span, density, rare, ex, ew)
    check_invariants(p, codes)
    return p


def oracle_weight(p: Planted) -> np.ndarray:
    """The planted layer through the ORACLE's dequantize (weight_values, orc_dequant_f32, the scale-dtype rounding, orc_svd_add, round,
    rotate_hadamard): float32 [N, K] values of T."""
    c = p.case
    vals = O.weight_values(p.stored, c.wdt, (c.n, c.k))
    gs = c.group
    if c.codebook:
        lv = p.scale.reshape(c.n, c.k // gs, -1)
        idx = vals.astype(np.int64).reshape(c.n, c.k // gs, gs)
        w = np.take_along_axis(lv, idx, axis=2).reshape(c.n, c.k)
    else:
        w = np.empty((c.n, c.k), dtype=np.float32)
        O.lib().orc_dequant_f32(O._p(O._c(vals, np.float32)), O._p(O._c(p.scale.reshape(-1), np.float32)),
                                O._p(None if p.zp is None else O._c(p.zp.reshape(-1), np.float32)), c.n, c.k, gs, O._p(w))
    if c.scale_tag != "f32":
        w = O.round_dtype(w, c.scale_tag)
    if c.rank:
        w = O._c(w, np.float32)
        O.lib().orc_svd_add(O._p(w), O._p(O._c(p.up, np.float32)), O._p(O._c(p.down, np.float32)), c.n, c.k, c.rank, O._DT[c.tag])
    w = O.round_dtype(w, c.tag)
    if c.had:
        w = O.rotate_hadamard(w, c.had, c.tag)
    return w


def check_invariants(p: Planted, codes=None):
    c = p.case
    tag = c.tag
    if codes is not None:  # the stored bytes decode to the chosen codes' values, by the oracle's convention
        vals = O.weight_values(p.stored, c.wdt, (c.n, c.k)).astype(np.float64)
        assert np.array_equal(vals, _code_values(c.wdt)[codes]), (c.id, "pack / weight_values round trip")
    assert representable(p.w_stored, tag) and representable(p.w, tag), (c.id, "a weight element is not a value of", tag)
    assert representable(p.x, tag) and all_normal(p.x, tag) and all_normal(p.w, tag) and all_normal(p.w_stored, tag), (c.id, "x / w not normal in", tag)
    for name, a in (("scale", p.scale), ("zero point", p.zp)):
        if a is not None:
            assert representable(a.astype(np.float64), c.scale_tag) and all_normal(a.astype(np.float64), c.scale_tag), (c.id, name)
    if p.up is not None:
        assert representable(p.up, tag) and representable(p.down, tag)
    if p.bias is not None:
        assert representable(p.bias, tag) and all_normal(p.bias, tag), (c.id, "bias")
        q = p.bias[None, :] / np.exp2((p.ex[:, None] + p.ew[None, :]).astype(np.float64))
        assert np.array_equal(q, np.rint(q)), (c.id, "the bias is off the grid of its column")
    assert p.span_bits <= BUDGET_BITS, (c.id, p.span_bits)
    y = p.expected()
    assert np.isfinite(y).all() and all_normal(y.astype(np.float64), tag), (c.id, "an expected output is not a normal number of", tag)


# ------------------------------------------------------------------------------------------------
# the three faults the exact-sum check must be able to see (tests/test_skinny_host.py)
# ------------------------------------------------------------------------------------------------
SWAP_A, TAIL_B = 5, 7  # the fixed pair of the swap: column 5 (first block) and column K - 7 (last 16-run, another block wherever K has two)


def _formed(p: Planted, w_stored: np.ndarray) -> np.ndarray:
    """The weight the kernel multiplies with, from an edited dequantized weight: un-rotated on Hadamard layers, where one stored element
    reaches its whole group."""
    return _unrotate(w_stored, p.case.had) if p.case.had else w_stored


def edit_one_code(p: Planted) -> np.ndarray:
    """Another code at ONE of the last 16 stored columns of every row (row n: column K - 1 - n % 16): a quarter of the code range (at least three steps) of the stored row's grid away.
    On a Hadamard layer the one code reaches its whole un-rotated group, 1 / sqrt(g) of the step each."""
    ws = p.w_stored.copy()
    steps = float(max(3, 1 << (O.dtype_info(p.case.wdt)["bits"] - 2)))
    rows = np.arange(p.case.n)
    ws[rows, p.case.k - 1 - rows % 16] += steps * np.exp2(_low_exp(p.w_stored, 1).astype(np.float64))
    return _formed(p, ws)


def edit_swap_columns(p: Planted) -> np.ndarray:
    """Stored columns 5 and K - 7 in each other's place: a fixed pair, in different chunks / blocks / ring slots wherever K has two."""
    ws = p.w_stored.copy()
    a, b = SWAP_A, p.case.k - TAIL_B
    ws[:, [a, b]] = ws[:, [b, a]]
    return _formed(p, ws)


def edit_zero_tail(p: Planted) -> np.ndarray:
    """The last live 16-run of the stored row never arrives."""
    ws = p.w_stored.copy()
    ws[:, -16:] = 0.0
    return _formed(p, ws)


EDITS = {"one code in the last 16 columns": edit_one_code, "two columns swapped": edit_swap_columns, "last 16-run zeroed": edit_zero_tail}


# ------------------------------------------------------------------------------------------------
# census columns
# ------------------------------------------------------------------------------------------------
def boundary_columns(kernel: str, k: int) -> np.ndarray:
    """First and last 16 columns of every pass / chunk / 256-group / 32-block, of every trip of the K loop and of the row."""
    cols = set()
    for step in {BLOCK[kernel], PERIOD[kernel]}:
        for b0 in range(0, k, step):
            b1 = min(b0 + step, k)
            cols.update(range(b0, min(b0 + 16, k)))
            cols.update(range(max(b1 - 16, 0), b1))
    cols.update(range(0, 16))
    cols.update(range(k - 16, k))
    return np.array(sorted(cols), dtype=np.int64)


# ------------------------------------------------------------------------------------------------
# device side (GPU tests only)
# ------------------------------------------------------------------------------------------------
def device_weight(p: Planted, device):
    """(QuantWeight built by ops.make_quant_weight from the planted tensors, svd_down_t [K, R] or None)."""
    from sdnq_amd import ops
    c = p.case
    dt, sdt = TAG_DT[c.tag], TAG_DT[c.scale_tag]
    t = lambda a, d: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(d).to(device)  # noqa: E731
    up, down = t(p.up, dt), t(p.down, dt)
    qw = ops.make_quant_weight(c.wdt, torch.from_numpy(p.stored).to(device), t(p.scale, sdt), t(p.zp, sdt), up, down, c.n, c.k, c.group,
                               transposed=False, codebook=c.codebook)
    return qw, (None if down is None else down.t().contiguous())


def device_x(x: np.ndarray, case: Case, device) -> torch.Tensor:
    """x [M, K] of T on the device as the case wants it: contiguous, a view of a wider matrix, or starting 8 bytes past a 16-byte boundary."""
    dt = TAG_DT[case.tag]
    m, k = x.shape
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(device)
    if case.strided:
        wide = torch.full((m, k + 64), 3.0, dtype=dt, device=device)  # the extra columns are live numbers: reading them shows
        wide[:, :k] = xt
        return wide[:, :k]
    if case.x_align != 16:
        assert dt.itemsize == 2 and case.x_align == 8
        buf = torch.zeros(m * k + 8, dtype=dt, device=device)
        view = buf[4:4 + m * k].view(m, k)
        view.copy_(xt)
        assert view.data_ptr() % 16 == 8
        return view
    return xt


def run(case: Case, qw, down_t, x: torch.Tensor, bias):
    from sdnq_amd import ops
    if case.rank:
        return ops.linear_skinny_svd(qw, down_t, x, bias)
    return ops.linear_skinny(qw, x, bias, case.had)


def census(case: Case, qw, down_t, cols: np.ndarray, device, m=None) -> np.ndarray:
    """The weight elements the kernel forms at `cols`: float32 [N, len(cols)].  Row i of a launch is one-hot (value 1) at its own column, there
    is no bias, so y[i][n] = w[n][col_i]; launches of `m` rows, the outputs stacked on the device and copied once."""
    m = case.m if m is None else m
    dt = TAG_DT[case.tag]
    launches = -(-len(cols) // m)
    x = torch.zeros((launches * m, case.k), dtype=dt, device=device)  # rows past the last column stay zero
    x[torch.arange(len(cols), device=device), torch.from_numpy(cols).to(device)] = 1.0
    plain = Case(case.kernel, case.wdt, case.gs, case.tag, m, case.k, had=case.had, rank=case.rank, scale_tag=case.scale_tag, codebook=case.codebook)
    outs = [run(plain, qw, down_t, x[i * m:(i + 1) * m], None) for i in range(launches)]
    return torch.cat(outs, 0)[:len(cols)].float().cpu().numpy().T


def first_mismatch(got: np.ndarray, want: np.ndarray):
    bad = np.argwhere(got != want)
    return (0, None) if bad.size == 0 else (len(bad), tuple(int(v) for v in bad[0]))


# ------------------------------------------------------------------------------------------------
# zero-point layers whose fma lands on a tie of T: the weight is rounded to float32 FIRST (dequantizer.py:27: addcmul in float32, then .to(T))
# ------------------------------------------------------------------------------------------------
TIE_CASES = (
    Case("fast", "uint8", 0, "f16", 2, 1040, note="tie"), Case("fast", "uint4", 16, "f16", 4, 1040, note="tie"),
    Case("generic", "uint7", 16, "f16", 3, 1040, note="tie"), Case("generic", "uint8", 0, "f16", 5, 1040, note="tie"),
    Case("svd", "uint8", 0, "f16", 2, 160, rank=16, note="tie"), Case("svd", "uint4", 32, "f16", 3, 160, rank=48, note="tie"),
    Case("svd32", "uint8", 0, "f16", 1, 640, rank=32, note="tie"), Case("svd32", "uint4", 64, "f16", 4, 576, rank=32, note="tie"),
    Case("svd32", "uint8", 32, "f16", 2, 544, rank=32, note="tie"), Case("svd32", "uint8", 0, "bf16", 4, 640, rank=32, note="tie"),
    Case("fast", "uint8", 0, "bf16", 1, 1040, note="tie"),
)


@functools.lru_cache(maxsize=16)
def plant_tie(case: Case) -> Planted:
    """z is the midpoint of two neighbours of T, s = +-2^-32: the exact q s + z lies a hair beside the tie, its float32 rounding ON it (q s is
    below half a float32 ulp of z), and the rounding to T then goes to the even neighbour.  Rounding the exact value to T at once -- what one
    fused fma-and-convert instruction does -- goes to the other neighbour wherever the hair points away from the even one.  The expected
    weight is the oracle's dequantize of the layer (`w`); `w_stored` holds that single-rounding model for the host test."""
    info = O.dtype_info(case.wdt)
    assert info["kind"] == "uint" and not case.had and not case.codebook
    rng = _rng(case, "tie")
    n, k, gs = case.n, case.k, case.group
    g_count = k // gs
    t = {"f16": 10, "bf16": 7}[case.tag]
    codes = rng.integers(0, 1 << info["bits"], size=(n, k))
    odd = rng.integers(0, 2, size=(n, g_count)) * 2 + 1                       # 1 + 2^-(t+1) | 1 + 3 * 2^-(t+1)
    z = (1.0 + odd * 2.0 ** -(t + 1)) * np.exp2(rng.integers(0, 2, size=(n, g_count)).astype(np.float64))
    s = np.where(rng.integers(0, 2, size=(n, g_count)) == 1, 1.0, -1.0) * 2.0 ** -32
    scale, zp = s.astype(np.float32), z.astype(np.float32)
    assert np.array_equal(scale.astype(np.float64), s) and np.array_equal(zp.astype(np.float64), z)
    up = down = None
    if case.rank:
        up, down = _svd(case)
    stored = _store(codes.reshape(-1), case.wdt)
    p = Planted(case, stored, scale, zp, up, down, None, None, None, None, 0, 0.0, 0.0)
    p.w = oracle_weight(p).astype(np.float64)
    exact = _code_values(case.wdt)[codes] * np.repeat(s, gs, axis=1) + np.repeat(z, gs, axis=1)  # exact in float64: 8 + 44 bits at most
    once = _round_once(exact, case.tag)
    p.w_stored = _round_once(once + up @ down, case.tag) if case.rank else once
    return p


def _round_once(a: np.ndarray, tag: str) -> np.ndarray:
    """float64 -> T in ONE rounding (round to nearest even on the T grid; values are normal in T)."""
    t = {"f16": 10, "bf16": 7}[tag]
    m, e = np.frexp(a)                      # a = m 2^e, 0.5 <= |m| < 1
    q = np.exp2((e - 1 - t).astype(np.float64))
    return np.rint(a / q) * q               # np.rint rounds half to even; a / q is exact (a power of two)
