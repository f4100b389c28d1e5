"""Bit-exact GPU tests of the many-row SVD branch: sdnq_hip_lowrank_down and the low-rank epilogue of the int8 / fp8 GEMM.

Every expected value comes from the CPU (tests/lowrank_util.py; tests/test_lowrank_exact_host.py checks two independent sources
against each other) and every comparison is np.array_equal / torch.equal on every output element: nothing here takes a tolerance.
Exact-sum inputs make bias + t . up^T exact in float32 in every order, so bias2d is one rounding of an exact value; the census inputs
(one product per output, arbitrary values) need not even that premise.

Which launcher condition sends a case to which path (gemm.hip, gemm_kernel's epilogue and launch_tiles<.., EPI_LOWRANK>):

  register layout                  lr_lds && zp == nullptr && a_zp == nullptr && svd dtype == output dtype, 16-bit output
                                   (lr_lds = rank == 32 && rank % 16 == 0 && svd dtype != float32): rank 32, bf16 -> bf16 and f16 -> f16
  staged, factors in LDS           lr_lds, but a float32 output, an output dtype other than the svd dtype, or a zero-point term:
                                   rank 32 with bf16 / f16 -> float32, bf16 -> f16, and every zero-point form at rank 32.  On the
                                   256x128 tile (forced id 3) a float32 output runs it in two chunks of 128 rows: 300 and 513 rows put
                                   rows into both
  staged, fragments from global    lr_mfma && rank != 32 (lr_mfma = rank % 16 == 0 && svd dtype != float32): ranks 16, 48, 64
  fmaf chain                       !lr_mfma: rank % 16 != 0 (8, 24, 40 with 16-bit factors) or float32 factors (rank 32)
  256x256 EPI_LRFAST, two chunks   heuristics only: tiles(256, 256) >= 160 && K >= 2048 && rank == 32 && svd dtype == output dtype (16 bits)
                                   && no zero-point term; ht_ok (K % 128 == 0) picks the half-tile ring, else the 64-byte pipeline.
                                   (2308, 3848, 2048) and (2308, 3848, 2064) are the smallest such shapes: 10 x 16 tiles, a tail of 4 rows
                                   and one of 8 columns.  sdnq_hip_scaled_mm_tile cannot probe a low-rank launch, so the rule is restated
                                   in lowrank_util.takes_lrfast and asserted
  bf16 scale chain (LP)            sdnq_hip_scaled_mm_lp / _lp_zp / _lp_uzp_svd: launch_lp -- 64x64 tiles up to 128 rows (M = 100), 64x128
                                   above (M = 300); the same four epilogue paths by the same conditions, every op rounded to bf16

Forced tiles (sdnq_hip_set_tile_override, reset by a fixture): 1 = 64x128, 2 = 64x64, 3 = 256x128, -1 = the heuristics (64x128 above
128 rows, 64x64 up to 128, for every small shape).  Id 0 is the same kernel as 3 for a low-rank epilogue and ids >= 4 are not
instantiated for it (PP_OK).

sdnq_hip_lowrank_down (linear_float.hip): 16-bit dtypes with K % 16 == 0 take the LDS-DMA ring kernel on v_mfma_f32_16x16x32_bf16 / _f16
-- RT = 2 row tiles per workgroup when ceil(ceil(M / 32) / 256) * 4 < ceil(ceil(M / 16) / 256) * 3, i.e. from 4097 rows on --, float32 and
K % 16 != 0 fall back to sdnq_hip_linear_float.  The adder span of the two 16x16x32 instructions was measured with
tools/micro/mfma_sum_probe.hip (profiles/mfma_sum_probe.txt): 23 bits, as for the 32x32 instructions, so the dense cases keep the
budget of exact_inputs.B (span - 2 bits, at most 20).
"""
import numpy as np
import pytest
import torch

from tests import exact_inputs as X
from tests import lowrank_util as L

pytestmark = pytest.mark.gpu

from sdnq_amd import _lib, ops  # noqa: E402

MM = {"int8": ops.MM_I8, "fp8": ops.MM_FP8}
MMS = ("int8", "fp8")


@pytest.fixture(autouse=True)
def default_tuning():
    L.require_default_tuning()


@pytest.fixture()
def tile_override():
    lib = _lib.load()
    yield lib.sdnq_hip_set_tile_override
    lib.sdnq_hip_set_tile_override(-1)


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _t(a: np.ndarray, dev, dtype=None) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


class _Resident:
    """One case's operands on the GPU."""

    def __init__(self, case: L.Case, dev):
        self.case = case
        self.a, self.b = case.main.a.to(dev), case.main.b.to(dev)
        self.sa, self.sb = _t(case.sa, dev), _t(case.sb, dev)
        self.t, self.up = case.t().to(dev), case.up().to(dev)
        self.bias = _t(case.bias, dev, L.DT[case.svd])   # values every 16-bit format holds: the cast is exact
        self.zero = {k: _t(v, dev) for k, v in case.zero.items()}

    def lowrank(self, with_bias: bool) -> torch.Tensor:
        z = self.zero
        return ops.scaled_mm_lowrank(MM[self.case.main.mm], self.a, self.b, self.sa, self.sb, self.bias if with_bias else None, self.t, self.up,
                                     z.get("rowsum"), z.get("zp"), L.DT[self.case.out], a_zp=z.get("a_zp"), w_colsum_scaled=z.get("wcs"))


def _msg(what, got, want) -> str:
    """Path, tile, shape and the first differing (m, n) with both values, as ONE string (pytest abbreviates a tuple's repr)."""
    return " ".join(str(w) for w in what) + ": " + L.where(got, want)


def _check(got, want, *what):
    assert np.array_equal(got, want), _msg(what, got, want)


# ---- 2. the GEMM epilogue on exact sums, per path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_id)
def test_epilogue_exact_sums_per_path(combo, mm, gpu_device, tile_override):
    """ops.scaled_mm_lowrank on the four ragged shapes, forced tiles 1 / 2 / 3 and the heuristics, with and without bias.
    Found by these cases: the register-layout path with float16 output (rank 32, f16 factors; the 256x256 EPI_LRFAST tiles too) let
    fma(acc sa, sb, bias2d) and the float16 conversion fold into one v_fma_mixlo_f16 -- one rounding where the reference rounds to
    float32 first.  [register_layout-r32-f16-f16-*] and test_epilogue_exact_sums_256x256_lrfast[*-f16-*] fail without the fix in
    gemm.hip (first seen at (300, 392, 528), tile 1, with bias)."""
    path, rank, svd, out = combo
    assert L.epilogue_path(rank, svd, out) == path
    for shape in L.SMALL_SHAPES:
        assert not L.takes_lrfast(*shape, rank, svd, out)
        res = _Resident(L.make_case(mm, *shape, rank, svd, out), gpu_device)
        want = {wb: res.case.expected(wb) for wb in (True, False)}
        for tile in L.TILES:
            tile_override(tile)
            for with_bias in (True, False):
                _check(_f32(res.lowrank(with_bias)), want[with_bias], path, mm, "tile", tile, shape, "bias", with_bias)


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("svd", ["bf16", "f16"])
@pytest.mark.parametrize("shape", L.LRFAST_SHAPES)
def test_epilogue_exact_sums_256x256_lrfast(shape, svd, mm, gpu_device):
    """The 256x256 EPI_LRFAST tiles (register layout in two chunks, the sr / trow row maps) under the default heuristics."""
    m, n, k = shape
    assert L.takes_lrfast(m, n, k, 32, svd, svd) and L.default_tile(m, n, 32, svd, svd, k) == (256, 256)
    assert L.lrfast_ring(k) == ("half-tile ring" if k == 2048 else "64-byte pipeline")
    case = L.make_case(mm, m, n, k, 32, svd, svd, check=False)
    rows = L.sample_rows(m, n, 32)
    assert L.sensitivity(case, True, rows) >= L.SENSITIVITY_FLOOR
    res = _Resident(case, gpu_device)
    for with_bias in (True, False):
        _check(_f32(res.lowrank(with_bias)), case.expected(with_bias), "256x256 EPI_LRFAST", L.lrfast_ring(k), mm, svd, shape, "bias", with_bias)


@pytest.mark.parametrize("svd", ["bf16", "f16"])
@pytest.mark.parametrize("form", L.ZERO_FORMS)
def test_epilogue_zero_point_forms_with_svd(form, svd, gpu_device, tile_override):
    """rowsum + zp (uint8 weights on the int8 matmul) and a_zp + w_colsum_scaled without / with zp (the uint8 matmul; zp_k = 0: the K of
    the K * (xzp * wzp) term is the launch's) against the float32 restatement of linear_int8.py:57-69 / linear_uint8.py:61-66."""
    for rank in (32, 16):
        path = L.epilogue_path(rank, svd, svd, zero_point=True)
        assert path == (L.STAGED_LDS if rank == 32 else L.STAGED_GLOBAL)
        for shape in ((300, 392, 528), (257, 264, 48)):
            res = _Resident(L.make_case("int8", *shape, rank, svd, svd, zero_form=form), gpu_device)
            want = {wb: res.case.expected(wb) for wb in (True, False)}
            for tile in (1, 3):
                tile_override(tile)
                for with_bias in (True, False):
                    _check(_f32(res.lowrank(with_bias)), want[with_bias], path, form, "tile", tile, shape, "rank", rank, "bias", with_bias)


# ---- the bf16 scale chain -------------------------------------------------------------------------------------------------------------
LP_SHAPES = ((100, 392, 528), (300, 392, 528))   # 64x64 tiles up to 128 rows, 64x128 above (launch_lp)


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("rank", [32, 16])
def test_bf16_scale_chain_lowrank_vs_oracle(rank, mm, gpu_device):
    """ops.scaled_mm_lp with t / svd_up against oracle.scaled_mm_lp with the 2-D bias."""
    for shape in LP_SHAPES:
        assert L.default_tile(shape[0], shape[1]) == ((64, 64) if shape[0] <= 128 else (64, 128))
        case = L.make_case(mm, *shape, rank, "bf16", "bf16", lp=True)
        res = _Resident(case, gpu_device)
        for with_bias in (True, False):
            got = ops.scaled_mm_lp(MM[mm], res.a, res.b, res.sa, res.sb, res.bias if with_bias else None, res.t, res.up)
            _check(_f32(got), case.expected_oracle(with_bias), "LP", L.epilogue_path(rank, "bf16", "bf16"), mm, shape, "rank", rank, "bias", with_bias)


@pytest.mark.parametrize("form", L.ZERO_FORMS)
@pytest.mark.parametrize("rank", [32, 16])
def test_bf16_scale_chain_zero_point_forms_with_svd(rank, form, gpu_device):
    """ops.scaled_mm_lp(..., rowsum, zp) and ops.scaled_mm_lp_uzp(..., t, svd_up) against the restatement that rounds to bf16 after
    every op."""
    for shape in LP_SHAPES:
        case = L.make_case("int8", *shape, rank, "bf16", "bf16", lp=True, zero_form=form)
        res = _Resident(case, gpu_device)
        z = res.zero
        for with_bias in (True, False):
            bias = res.bias if with_bias else None
            if form == "rowsum+zp":
                got = ops.scaled_mm_lp(ops.MM_I8, res.a, res.b, res.sa, res.sb, bias, res.t, res.up, rowsum=z["rowsum"], zp=z["zp"])
            else:
                got = ops.scaled_mm_lp_uzp(res.a, res.b, res.sa, res.sb, bias, z.get("rowsum"), z.get("zp"), z["a_zp"], z["wcs"], 0, res.t, res.up)
            _check(_f32(got), case.expected(with_bias), "LP", L.epilogue_path(rank, "bf16", "bf16", True), form, shape, "rank", rank, "bias", with_bias)


# ---- 3. the factor census -------------------------------------------------------------------------------------------------------------
def _census(mm, m, n, k, rank, svd, out, transposed, dev, tiles, override, what):
    main = L.main_operands(mm, m, n, k, zero=True)
    a, b = main.a.to(dev), main.b.to(dev)
    rng = np.random.default_rng(m + n)
    sa, sb = _t(rng.uniform(0.01, 2.0, size=m).astype(np.float32), dev), _t(rng.uniform(0.01, 2.0, size=n).astype(np.float32), dev)
    for shift in range(rank):
        t, up, prod = L.factor_census(m, n, rank, shift, svd, transposed)
        want = L.bits(L.census_expected(prod, svd, out))
        td, upd = t.to(dev), up.to(dev)
        for tile in tiles:
            if override is not None:
                override(tile)
            got = L.bits(ops.scaled_mm_lowrank(MM[mm], a, b, sa, sb, None, td, upd, None, None, L.DT[out]))
            if not np.array_equal(got, want):
                f = lambda b: torch.from_numpy(b).view(L.DT[out]).float().numpy()  # noqa: E731
                pytest.fail(_msg((*what, "tile", tile, (m, n, k), "shift", shift, "one-hot svd_up" if transposed else "one-hot t"), f(got), f(want)))


@pytest.mark.parametrize("transposed", [False, True], ids=["one_hot_t", "one_hot_up"])
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_id)
def test_epilogue_factor_census_per_path(combo, transposed, gpu_device, tile_override):
    """All-zero activations and no bias: out == cast_out(cast_svd(ONE product)), with the one-hot column moved over all R so that
    every (32-row block, rank column) pair is read back -- on the 64x128 and the 256x128 tile."""
    path, rank, svd, out = combo
    mm = "fp8" if rank in (16, 24) else "int8"
    _census(mm, 300, 392, 64, rank, svd, out, transposed, gpu_device, (1, 3), tile_override, (path, mm))


@pytest.mark.parametrize("transposed", [False, True], ids=["one_hot_t", "one_hot_up"])
@pytest.mark.parametrize("svd", ["bf16", "f16"])
def test_epilogue_factor_census_256x256_lrfast(svd, transposed, gpu_device):
    m, n, k = L.LRFAST_SHAPES[0]
    assert L.takes_lrfast(m, n, k, 32, svd, svd)
    _census("int8", m, n, k, 32, svd, svd, transposed, gpu_device, (-1,), None, ("256x256 EPI_LRFAST", L.lrfast_ring(k)))


# ---- 4. lowrank_down ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lowrank_down_exact_sums(fmt, gpu_device):
    """t = round_T(float64 sum) on exact-sum x and svd_down.  (5, 16, 8) .. (64, 112, 40): K below / at / across 128-element stages
    (zero-filled DMAs past K), R below 32, R = 48 and 40 (a second N tile with 16 / 8 live rows), R = 64; (4100, 272, 32) and
    (8192, 144, 32) take RT = 2 -- 4100 rows leave the last workgroup 4 live rows and one whole dead row tile, 8192 fill 256
    workgroups exactly, the last M of one round.  (By the launcher's rule, restated in lowrank_util.lrd_row_tiles and asserted here,
    every M above 4096 takes RT = 2, not only those up to 8192.)"""
    assert X.MEASURED_SPAN_BITS[L.DOWN_MFMA[fmt]] == 23
    for m, k, r in L.DOWN_SHAPES:
        assert L.lrd_row_tiles(m) == (2 if m > 4096 else 1) and k % 16 == 0
        ex, want = L.down_case(m, k, r, fmt)
        got = _f32(ops.lowrank_down(ex.a.to(gpu_device), ex.b.to(gpu_device)))
        _check(got, want, "lowrank_down", fmt, (m, k, r), "RT", L.lrd_row_tiles(m))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lowrank_down_column_view_zero_row_and_k200(fmt, gpu_device):
    """x as a column view of a wider activation (ldx > K, a 16-byte aligned offset, arbitrary values beside it); a row of zeros stays
    zero; K = 200 (K % 16 != 0) takes the 16-bit fallback, sdnq_hip_linear_float."""
    m, k, r = 257, 400, 48
    ex, want = L.down_case(m, k, r, fmt)
    wide = X._arbitrary(np.random.default_rng(1), (m, k + 48), fmt)
    wide[:, 8:8 + k] = ex.a
    view = wide.to(gpu_device)[:, 8:8 + k]
    assert view.stride(0) == k + 48 and view.data_ptr() % 16 == 0
    _check(_f32(ops.lowrank_down(view, ex.b.to(gpu_device))), want, "lowrank_down", fmt, "column view", (m, k, r))
    x0 = ex.a.clone()
    x0[100] = 0
    got = _f32(ops.lowrank_down(x0.to(gpu_device), ex.b.to(gpu_device)))
    assert not got[100].any(), f"lowrank_down {fmt} zero row: {got[100]}"
    keep = np.arange(m) != 100
    _check(got[keep], want[keep], "lowrank_down", fmt, "rows beside the zero row")
    ex2, want2 = L.down_case(100, 200, 16, fmt)
    _check(_f32(ops.lowrank_down(ex2.a.to(gpu_device), ex2.b.to(gpu_device))), want2, "lowrank_down", fmt, "K = 200 fallback", (100, 200, 16))


@pytest.mark.parametrize("transposed", [False, True], ids=["one_hot_x", "one_hot_down"])
@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_lowrank_down_k_census(fmt, transposed, gpu_device):
    """x one-hot (1.0 at column (row * 9 + shift) % K) for EVERY shift: every k of every 128-element stage and 8-element chunk is read
    back through every row of a 16-row tile, and t[m][r] must be svd_down[r][k] bit for bit; then one-hot rows of svd_down against
    arbitrary x.  float32 (the fallback to sdnq_hip_linear_float: its MFMA GEMM above 32 rows, the few-row kernel below) gets the
    census only -- its adder span is unmeasured."""
    shapes = ((77, 16, 8), (77, 400, 48)) if fmt != "f32" else ((77, 16, 8), (77, 400, 48), (20, 400, 48))
    for m, k, r in shapes:
        for shift in range(k):
            x, down, want = L.down_census(m, k, r, shift, 9, fmt, transposed)
            got = ops.lowrank_down(x.to(gpu_device), down.to(gpu_device))
            assert np.array_equal(L.bits(got), L.bits(want)), _msg(("lowrank_down", fmt, (m, k, r), "shift", shift,
                                                                    "one-hot svd_down" if transposed else "one-hot x"), _f32(got), _f32(want))
