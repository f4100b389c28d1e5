"""CPU checks of tests/lowrank_util.py: the expected values of the low-rank (SVD) branch's bit-exact GPU tests
(tests/test_lowrank_exact_gpu.py) are what they claim to be, and a subtly wrong kernel could not pass them.  Nothing here needs a GPU.

 * two independent sources of the expected output agree bit for bit on every small case of the path table: the C oracle
   (lowrank_bias, then scaled_mm / scaled_mm_lp with the 2-D bias) and the float64 sums rounded once pushed through
   exact_inputs.epilogue / the float32 restatement;
 * the float32 restatement of the zero-point forms reproduces oracle.forward on the epilogue inputs of the SVD fixtures that carry
   zero-point terms;
 * the sensitivity condition holds for every case; modelled faults change the expected bits of every row they touch.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import exact_inputs as X
from tests import lowrank_util as L
from tests.golden_util import Case as Golden

MMS = ("int8", "fp8")


def test_path_table_follows_the_launcher_rules():
    for path, rank, svd, out in L.COMBOS:
        assert L.epilogue_path(rank, svd, out) == path, (path, rank, svd, out)
    # a zero-point term takes the register layout away from rank 32, and leaves the other paths where they are
    assert L.epilogue_path(32, "bf16", "bf16", zero_point=True) == L.STAGED_LDS
    assert L.epilogue_path(16, "bf16", "bf16", zero_point=True) == L.STAGED_GLOBAL
    for m, n, k in L.SMALL_SHAPES:
        assert not L.takes_lrfast(m, n, k, 32, "bf16", "bf16")
        assert L.default_tile(m, n, k=k) == ((64, 128) if m > 128 else (64, 64))
    (m, n, k0), (_, _, k1) = L.LRFAST_SHAPES
    for svd in ("bf16", "f16"):
        assert L.takes_lrfast(m, n, k0, 32, svd, svd) and L.takes_lrfast(m, n, k1, 32, svd, svd)
    assert L.lrfast_ring(k0) == "half-tile ring" and L.lrfast_ring(k1) == "64-byte pipeline"
    # the smallest such shape: one tile row or column less, or a shorter K, and the launcher stays on the small tiles
    assert not L.takes_lrfast(m - 4, n, k0, 32, "bf16", "bf16") and not L.takes_lrfast(m, n - 8, k0, 32, "bf16", "bf16")
    assert not L.takes_lrfast(m, n, k0 - 16, 32, "bf16", "bf16") and not L.takes_lrfast(m, n, k0, 32, "bf16", "f32")
    assert m % 256 == 4 and n % 256 == 8 and k0 % 16 == 0 and k1 % 16 == 0 and n % 8 == 0
    # lowrank_down: two row tiles per workgroup from 4097 rows on; 4100 rows leave the last workgroup 4 live rows and a dead tile
    assert [L.lrd_row_tiles(r) for r in (5, 257, 4096, 4097, 4100, 8192)] == [1, 1, 1, 2, 2, 2]
    assert 4100 % 32 == 4 and 8192 // 32 == 256


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("combo", L.COMBOS, ids=L.combo_id)
def test_two_sources_of_the_expected_output_agree_and_cases_are_sensitive(combo, mm):
    """Per small case: the C oracle == float64 sums rounded once + the float32 epilogue, with and without bias; bias2d is one rounding
    of an exact value (round_to asserts it); dropping a rank column changes at least half of every (sampled) row's outputs."""
    _, rank, svd, out = combo
    for shape in L.SMALL_SHAPES:
        case = L.make_case(mm, *shape, rank, svd, out)
        assert case.share >= L.SENSITIVITY_FLOOR, (shape, case.share)
        for with_bias in (True, False):
            assert np.array_equal(case.bias2d(with_bias), case.bias2d_oracle(with_bias)), (shape, with_bias)
            want, ref = case.expected(with_bias), case.expected_oracle(with_bias)
            assert np.array_equal(want, ref), (shape, with_bias, L.where(want, ref))
            general = L.restated_epilogue(case.main.acc, case.sa, case.sb, case.bias2d(with_bias), out)
            assert np.array_equal(general, want), (shape, with_bias, L.where(general, want))
        # the low-rank term matters: without it the output is another one nearly everywhere
        plain = X.epilogue(case.main.acc, case.sa, case.sb, case.bias, out)
        assert (plain != case.expected(True)).mean() > 0.9, shape


@pytest.mark.parametrize("svd", ["bf16", "f16"])
@pytest.mark.parametrize("m,n,k,rank", [(300, 392, 528, 32), (257, 264, 48, 16), (33, 72, 16, 48)])
def test_sensitivity_on_every_row(m, n, k, rank, svd):
    """The builder samples rows once m n rank passes SENSITIVITY_WORK; here EVERY row of three cases, int8 codes in +-127: zeroing any
    rank column over any 32-row block changes at least half of the outputs of every row of that block, and no row stays unchanged."""
    case = L.make_case("int8", m, n, k, rank, svd, svd)
    for with_bias in (True, False):
        assert L.sensitivity(case, with_bias) >= L.SENSITIVITY_FLOOR, (with_bias, L.sensitivity(case, with_bias))


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("m,n,k,rank", [(100, 392, 528, 32), (300, 392, 528, 32), (100, 264, 48, 16), (300, 264, 48, 16)])
def test_bf16_scale_chain_sources_agree(m, n, k, rank, mm):
    """The bf16 scale chain: oracle.scaled_mm_lp with the 2-D bias == the restatement that rounds to bf16 after every op."""
    case = L.make_case(mm, m, n, k, rank, "bf16", "bf16", lp=True)
    assert case.share >= L.SENSITIVITY_FLOOR
    for scale in (case.sa, case.sb):
        assert np.array_equal(np.exp2(np.round(np.log2(scale))), scale), "power-of-two scales"
    for with_bias in (True, False):
        want, ref = case.expected(with_bias), case.expected_oracle(with_bias)
        assert np.array_equal(want, ref), (with_bias, L.where(want, ref))


@pytest.mark.parametrize("lp", [False, True])
@pytest.mark.parametrize("form", L.ZERO_FORMS)
def test_zero_point_cases_are_sensitive_and_every_term_matters(form, lp):
    for rank in (32, 16):
        case = L.make_case("int8", 300, 392, 528, rank, "bf16", "bf16", lp=lp, zero_form=form)
        assert case.share >= L.SENSITIVITY_FLOOR
        want = case.expected(True)
        k = case.shape[2]
        for name in case.zero:   # a term lost, or scaled by the wrong row / column, is another output
            if name == "rowsum":
                other = dict(case.zero, rowsum=np.roll(case.zero["rowsum"], 1))
            else:
                other = dict(case.zero, **{name: np.roll(case.zero[name], 1)})
            got = L.restated_epilogue(case.main.acc, case.sa, case.sb, case.bias2d(True), "bf16", lp, k=k, **other)
            assert ((got != want).mean(axis=1) > 0).mean() > 0.9, (form, lp, name)
        if "zp" in case.zero and "a_zp" in case.zero:   # the K of the K * (xzp * wzp) term
            got = L.restated_epilogue(case.main.acc, case.sa, case.sb, case.bias2d(True), "bf16", lp, k=k - 16, **case.zero)
            assert (got != want).mean() > 0.25, (form, lp)


def _fixture_epilogue_inputs(c: Golden):
    """The operands of the fixture's scaled matmul as oracle.forward prepares them (linear_int8.py:38-69, linear_uint8.py:27-66)."""
    mod = c.oracle_module()
    d, f = mod.deq, np.float32
    m = c.ms()[-1]
    x = c.f32(f"x_{m}")
    x2 = np.ascontiguousarray(x.reshape(-1, mod.K), dtype=f)
    lp = mod.scale_tag != "f32"
    r = L._rb if lp else (lambda v: np.asarray(v, dtype=f))
    if d["use_hadamard"]:
        x2 = O.rotate_hadamard(x2, d["hadamard_group_size"], c.tag)
    up, down = mod.svd_nr_rk()
    t = O.linear_float(O.round_dtype(x2, mod.svd_tag), down, None, mod.svd_tag)
    bias2d = O.lowrank_bias(t, up, None if mod.bias is None else O.round_dtype(mod.bias, mod.svd_tag), mod.svd_tag)
    kw = {}
    if d["quantized_matmul_dtype"] == "uint8":
        if d["re_quantize_for_matmul"]:
            wq, sc, zp = mod.re_quantize_matmul()
        else:
            vals, sc, zpv, _ = mod._nk_values_scale()
            sc = sc.reshape(-1)
            wq = (vals.astype(np.int32).astype(np.uint8) ^ 0x80).view(np.int8)
            zp = r(zpv.reshape(-1) + f(128.0) * sc)
        q, xs, xzp = O.rowquant_asym_lp(x2, "bf16") if lp else O.rowquant_asym(x2)
        kw = dict(rowsum=q.astype(np.int32).sum(-1), zp=zp, a_zp=xzp, wcs=r(r(wq.astype(np.int32).sum(-1).astype(f)) * sc))
    else:
        wq, sc, zp = O._mm_weights(mod, "int8")
        if lp:
            zp = O.round_dtype(zp, mod.scale_tag)
        q, xs, rowsum = O.rowquant_lp(x2, "int8", mod.scale_tag) if lp else O.rowquant(x2, "int8")
        kw = dict(rowsum=rowsum, zp=zp)
    acc = X.int_matmul(q.astype(np.int64), wq.astype(np.int64)).astype(np.float64)
    return mod, x, acc, xs, sc, bias2d, lp, kw


@pytest.mark.parametrize("name", ["uint8_svd32_int8mm_qmm_bf16_lpscale", "uint8_svd32_uint8mm_qmm_bf16_lpscale", "int4_svd_had_uint8mm_qmm_f16"])
def test_zero_point_restatement_reproduces_oracle_forward_on_svd_fixtures(name):
    """On the fixtures' own epilogue inputs -- the bias2d the oracle computed included -- the restatement equals oracle.forward on EVERY
    element: the order of the low-rank sum does not enter, because bias2d is taken as an input here, exactly as the kernel's staged
    paths take it from their MFMAs.  (The two uint8-weight fixtures run the bf16 chain, the int4 one the float32 chain of the uint8
    matmul with a weight zero point.)"""
    c = Golden(name)
    mod, x, acc, xs, sc, bias2d, lp, kw = _fixture_epilogue_inputs(c)
    want = O.forward(mod, x, c.tag).reshape(acc.shape)
    got = L.restated_epilogue(acc, xs, sc, bias2d, c.tag, lp, k=mod.K, **kw)
    assert np.array_equal(got, want), (name, L.where(got, want))


def _first_case(mm="int8", rank=32, svd="bf16", out="bf16", shape=(300, 392, 528)):
    return L.make_case(mm, *shape, rank, svd, out)


def _assert_every_touched_row_changes(got, want, rows, what):
    assert len(rows) > 0, what
    changed = (got[rows] != want[rows]).any(axis=1)
    assert changed.all(), (what, "rows that keep every bit:", rows[~changed][:8])


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("svd", ["bf16", "f16"])
@pytest.mark.parametrize("with_bias", [True, False])
def test_modelled_epilogue_faults_change_every_touched_row(with_bias, svd, mm):
    """What a subtly wrong low-rank epilogue would write differs from the expected bits in every row it touches."""
    for rank, shape in ((32, (300, 392, 528)), (16, (257, 264, 48)), (48, (33, 72, 16))):
        case = _first_case(mm, rank, svd, svd, shape)
        want = case.expected(with_bias)
        m = shape[0]
        for block in (0, (m - 1) // 32):          # the first 32-row block and the ragged last one
            for col in (0, 7, 8, rank - 1):
                got, rows = L.fault_drop_rank_column(case, block, col, with_bias)
                _assert_every_touched_row_changes(got, want, rows, ("dropped rank column", block, col))
            got, rows = L.fault_t_row_32_down(case, block, with_bias)
            if len(rows):
                _assert_every_touched_row_changes(got, want, rows, ("t row from 32 rows further down", block))
        for step in range(rank // 16):
            got, rows = L.fault_swap_rank_halves(case, step, with_bias)
            _assert_every_touched_row_changes(got, want, rows, ("swapped 8-element rank halves", step))
        got, rows = L.fault_up_row_4_on(case, with_bias)
        _assert_every_touched_row_changes(got, want, rows, "svd_up row n + 4")


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lowrank_down_expected_values_and_lost_chunk(fmt):
    """round_T(float64 sum) == the oracle's float linear on the exact-sum operands; a lost last K chunk of svd_down changes every row
    that has a nonzero activation there."""
    for m, k, r in L.DOWN_SHAPES + ((100, 200, 16),):
        if m * k * r > 20_000_000:
            continue   # the two RT = 2 shapes: the same construction, checked on the GPU against the float64 sums
        ex, want = L.down_case(m, k, r, fmt)
        ref = O.linear_float(*ex.codes(), None, fmt)
        assert np.array_equal(want, ref), ((m, k, r), L.where(want, ref))
        got, rows = L.fault_down_lost_last_chunk(ex, fmt)
        _assert_every_touched_row_changes(got, want, rows, ("lost last chunk", (m, k, r)))


@pytest.mark.parametrize("svd", ["bf16", "f16", "f32"])
def test_census_products_are_exact_and_cover_every_rank_column(svd):
    m, n, rank = 300, 392, 64
    seen_t, seen_up = np.zeros((-(-m // 32), rank), dtype=bool), np.zeros((-(-n // 32), rank), dtype=bool)
    for shift in range(rank):
        for transposed in (False, True):
            t, up, prod = L.factor_census(m, n, rank, shift, svd, transposed)
            exact = t.double() @ up.double().T   # one nonzero product per output
            assert torch.equal(prod.double(), exact) and bool((prod != 0).all()), (shift, transposed)
            hot = up if transposed else t
            assert bool(((hot != 0).sum(1) == 1).all())
            rows, cols = np.nonzero(hot.float().numpy())
            (seen_up if transposed else seen_t)[rows // 32, cols] = True
            lo = L.census_expected(prod, svd, "f16" if svd == "f16" else "bf16").float().abs()
            assert bool(torch.isfinite(lo).all()) and float(lo.min()) >= 2.0 ** -7, "window keeps every product normal"
    assert seen_t.all() and seen_up.all(), "every (32-row block, rank column) pair is read back"


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_lowrank_down_census_covers_every_k(fmt):
    m, k, r, stride = 77, 400, 48, 9
    hit = np.zeros((16, k), dtype=bool)
    for shift in range(k):
        x, down, want = L.down_census(m, k, r, shift, stride, fmt, False)
        rows, cols = np.nonzero(x.float().numpy())
        assert len(rows) == m
        hit[rows % 16, cols] = True
        assert torch.equal(want.double(), x.double() @ down.double().T)
    assert hit.all(), "every k is read back through every row of a 16-row tile"
    x, down, want = L.down_census(m, k, r, 5, stride, fmt, True)
    assert torch.equal(want.double(), x.double() @ down.double().T)
