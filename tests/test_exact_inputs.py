"""CPU checks of tests/exact_inputs.py: the exact-sum operands are what they claim to be, the CPU oracle is bit-exact on them, and a
subtly wrong kernel could not pass the GPU tests built on them (tests/test_exact_sums_gpu.py).  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import exact_inputs as X

FMTS = ("fp8", "bf16", "f16")
SMALL = tuple(s for s in X.RAGGED_SHAPES if s[0] * s[1] * s[2] <= 140_000_000)  # the oracle-backed checks: the shapes a CPU does in a blink


def _ex(shape, fmt, seed=1):
    return X.exact_operands(*shape, seed=seed, fmt=fmt)


def test_budget_comes_from_the_recorded_probe():
    """B = measured span - 2 bits, at most 20; the spans are the ones profiles/mfma_sum_probe.txt records."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mfma_sum_probe.txt")
    spans = [int(v) for v in re.findall(r"measured span, accumulator against products \(a, b\): (\d+) bits", open(path).read())]
    probed = FMTS + ("bf16_16x16x32", "f16_16x16x32")  # the file's order: the GEMMs' three instructions, then lowrank_down's two
    assert spans == [X.MEASURED_SPAN_BITS[f] for f in probed]
    assert X.B == {f: min(X.MEASURED_SPAN_BITS[f] - 2, 20) for f in probed}
    assert min(spans) >= 10  # below that the dense cases would have to fall back to {0, +-1} values and K <= 512


@pytest.mark.parametrize("fmt", FMTS)
def test_every_value_survives_its_dtype(fmt):
    for shape in X.RAGGED_SHAPES:
        ex = _ex(shape, fmt)
        for t, ints, e in ((ex.a, ex.ia, ex.ea), (ex.b, ex.ib, ex.eb)):
            want = ints.astype(np.float64) * np.exp2(e.astype(np.float64))[:, None]
            assert np.array_equal(t.float().numpy().astype(np.float64), want), (fmt, shape)
            assert np.abs(ints).max() <= X.IMAX and (ints != 0).mean() >= 0.25
        lo, hi = X.E_WINDOW[fmt]
        assert lo <= ex.ea.min() and ex.ea.max() <= hi and lo <= ex.eb.min() and ex.eb.max() <= hi
    # the window's ends: e4m3 subnormals (multiples of 2^-9) and 4 * 2^6; the 16-bit windows stay normal
    lo, hi = X.E_WINDOW[fmt]
    edge = X.to_format(np.array([[1, 3, 4, -4]]), np.array([lo]), fmt).float().numpy()
    assert np.array_equal(edge, np.array([[1, 3, 4, -4]], dtype=np.float32) * np.float32(2.0 ** lo))
    assert float(X.to_format(np.array([[4]]), np.array([hi]), fmt).float()) == 4 * 2.0 ** hi
    if fmt != "fp8":
        assert 2.0 ** lo >= float(torch.finfo(X.TORCH_DT[fmt]).tiny)
    for shift in X.one_hot_shifts(208):
        oh = X.one_hot_operands(100, 136, 208, shift, fmt)
        a = oh.a.float().numpy()
        assert np.isfinite(a).all() and np.isfinite(oh.b.float().numpy()).all()
        assert ((a != 0).sum(1) == 1).all() and (a[np.arange(100), oh.cols] != 0).all() and oh.cols[0] == shift


@pytest.mark.parametrize("fmt", FMTS)
def test_span_within_budget_and_outputs_dense(fmt):
    for shape in X.RAGGED_SHAPES + X.W8A16_SHAPES + X.FLOAT_EXTRA_SHAPES:
        ex = _ex(shape, fmt)
        assert ex.span_bits == X.span_bits_of(ex.ia, ex.ib) <= X.B[fmt], (fmt, shape, ex.span_bits)
        terms = X.int_matmul((ex.ia != 0).astype(np.int64), (ex.ib != 0).astype(np.int64))
        assert int(terms.min()) * 32 >= shape[2], (fmt, shape, int(terms.min()))
    with pytest.raises(ValueError):
        X.exact_operands(64, 64, 64, 0, fmt, density=0.1)  # too sparse: rejected, not patched up


def test_span_bound_of_the_model_size_operands():
    """Model size: the m x n x k product of magnitudes is replaced by a rigorous upper bound; it is one (checked on a shape where both
    are cheap) and it fits the budget on every model-size shape."""
    ex = _ex((300, 392, 528), "fp8")
    assert X.span_bits_of(ex.ia, ex.ib, exact=False) >= ex.span_bits
    for (m, n, k) in X.MODEL_SHAPES:
        rng = np.random.default_rng(k)
        ia, ib = X._draw(rng, 64, k, X.density_for(k)), X._draw(rng, 64, k, X.density_for(k))
        assert X.span_bits_of(ia, ib, exact=False) <= np.ceil(np.log2(X.IMAX * X.IMAX * k)) <= X.B["fp8"]


@pytest.mark.parametrize("tag", ["bf16", "f16", "f32"])
def test_oracle_equals_int64_sums_through_the_epilogue(tag):
    for shape in SMALL:
        m, n, k = shape
        rng = np.random.default_rng(m + n)
        sa = (rng.random(m) * 0.02 + 1e-4).astype(np.float32)
        sb = (rng.random(n) * 0.02 + 1e-4).astype(np.float32)
        bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(torch.bfloat16).float().numpy()
        ex = _ex(shape, "fp8")
        ac, bc = ex.codes()
        cases = [(ac, bc, ex.acc())]
        oh = X.one_hot_operands(m, n, k, k - 1, "fp8")
        cases.append((*oh.codes(), oh.acc()))
        for (a, b, acc) in cases:
            for bs in (bias, None):
                ref = O.scaled_mm("fp8", a, b, sa, sb, bs, tag)
                assert np.array_equal(ref, X.epilogue(acc, sa, sb, bs, tag)), (shape, tag, bs is None)
                assert np.isfinite(ref).all()
        if tag == "f32":
            continue
        # the float-linear oracle: accumulator + bias, one rounding
        ex = _ex(shape, tag)
        bias = X.exact_bias(ex, 3)
        xa, wb = ex.codes()
        for bs in (bias, None):
            want = ex.acc() + (0.0 if bs is None else bs.astype(np.float64)[None, :])
            want32 = want.astype(np.float32)
            assert np.array_equal(want32.astype(np.float64), want)  # exact in float32: the kernel's fp32 add cannot round
            want_t = torch.from_numpy(want32).to(X.TAG_DT[tag]).float().numpy()
            ref = O.linear_float(xa, wb, bs, tag)
            assert np.array_equal(ref, want_t) and np.isfinite(ref).all(), (shape, tag)


def test_fma_model_rounds_once():
    """_fma_f32 against exact rational arithmetic: the result is the float32 nearest to v * s + c, also where |c| dwarfs the product
    (the low bits of the product then lie below float64's last place, where a plain float64 sum would round twice)."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    v = rng.standard_normal(1500).astype(np.float32)
    s = rng.standard_normal(1500).astype(np.float32)
    c = (rng.standard_normal(1500) * np.exp2(rng.integers(-30, 40, size=1500))).astype(np.float32)
    got = X._fma_f32(v, s, c)
    for i in range(1500):
        exact = Fraction(float(v[i])) * Fraction(float(s[i])) + Fraction(float(c[i]))
        d = abs(Fraction(float(got[i])) - exact)
        for other in (np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))):
            assert d <= abs(Fraction(float(other)) - exact), i


@pytest.mark.parametrize("fmt", FMTS)
def test_a_subtly_wrong_kernel_could_not_pass(fmt):
    """Three faults of a GEMM's K handling, applied to the CPU model: a dropped K element, two 16-byte K chunks of B read in each
    other's place, the last 16-byte chunk of a K tail counted twice.  On every shape the GPU tests use, each changes the exact
    accumulator -- the float32 output -- of at least one element in EVERY row it touches, and the bf16 / f16 output (which rounds
    differences of less than 2^-8 / 2^-11 of an output away) in most of them; the one-hot operands, where an output IS one product,
    change in the 16-bit outputs too."""
    ce = X.chunk_elems(fmt)
    for shape in X.RAGGED_SHAPES + X.W8A16_SHAPES + X.FLOAT_EXTRA_SHAPES:
        m, n, k = shape
        ex = _ex(shape, fmt)
        good = X.expected_int(ex.ia, ex.ib)
        faults = [("drop first", *X.corrupt_drop(ex, 0)), ("drop last", *X.corrupt_drop(ex, k - 1)), ("drop middle", *X.corrupt_drop(ex, k // 2)),
                  ("tail twice", *X.corrupt_double_tail(ex))]
        if k >= 2 * ce:
            faults.append(("swap chunks", *X.corrupt_swap_b_chunks(ex, 0, k // ce - 1)))
            faults.append(("swap neighbours", *X.corrupt_swap_b_chunks(ex, k // ce - 2, k // ce - 1)))
        scale = np.exp2((ex.ea[:, None] + ex.eb[None, :]).astype(np.float64))
        tag = "bf16" if fmt == "fp8" else fmt
        good16 = torch.from_numpy((good * scale).astype(np.float32)).to(X.TAG_DT[tag])
        for name, bad, rows in faults:
            assert len(rows) >= m // 8, (fmt, shape, name, "touches too few rows to mean anything")
            changed = (bad != good).any(1)
            assert changed[rows].all(), (fmt, shape, name, "rows a float32 output would not notice", int((~changed[rows]).sum()))
            assert not np.delete(changed, rows).any()
            bad16 = torch.from_numpy((bad * scale).astype(np.float32)).to(X.TAG_DT[tag])
            changed16 = (bad16 != good16).any(1).numpy()
            assert changed16[rows].mean() >= 0.9, (fmt, shape, name, "16-bit output", float(changed16[rows].mean()))
        # one product per output: losing or mis-pairing it changes the 16-bit output itself
        oh = X.one_hot_operands(m, n, k, k - 1, fmt)
        a, b = oh.a.float().numpy().astype(np.float64), oh.b.float().numpy().astype(np.float64)
        good1 = torch.from_numpy(oh.acc().astype(np.float32)).to(X.TAG_DT[tag])
        kk = int(oh.cols[0])
        a_drop = a.copy()
        a_drop[:, kk] = 0
        rows = np.nonzero(oh.cols == kk)[0]
        bad1 = torch.from_numpy((a_drop @ b.T).astype(np.float32)).to(X.TAG_DT[tag])
        assert (bad1 != good1).any(1).numpy()[rows].all()
        if k >= 2 * ce:
            b_swap = b.copy()
            b_swap[:, :ce], b_swap[:, k - ce:] = b[:, k - ce:], b[:, :ce]
            rows = np.nonzero((oh.cols < ce) | (oh.cols >= k - ce))[0]
            bad1 = torch.from_numpy((a @ b_swap.T).astype(np.float32)).to(X.TAG_DT[tag])
            assert len(rows) and (bad1 != good1).any(1).numpy()[rows].all()
