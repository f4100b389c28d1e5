"""CPU checks of tests/hadamard_exact.py: the integer expectation IS the oracle's (and the reference's) rotation on the generator's rows, the
case tables of the GPU file name every kernel form the row quantizer's dispatcher can pick, and the exact comparison sees the faults a
hand-written rotation can have (a numpy model of the butterflies with one fault each)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hadamard_exact as H
from tests.skinny_util import _round_once


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("tag", H.TAGS)
@pytest.mark.parametrize("g", H.GROUPS)
def test_expected_rotation_is_the_oracles(g, tag):
    for amp in (8, 64, None):
        x = H.exact_rows(37, 3 * g, tag, 1, amp, g)
        want = H.expected_rotation(x, g, tag)
        assert _same(want, O.rotate_hadamard(x, g, tag)), (g, tag, amp)
        if amp is None and H.rounding_can_show(g, tag):
            assert H.inexact_share(x, g, tag) >= 0.5
        if H.is_pow4(g) or tag != "f32":
            # the reference's formulation: x.view(-1, g) @ H with H = +-c in the dtype, float32 accumulation, one rounding -- here the sum in
            # float64 (exact: 24 + 24 bits), rounded ONCE
            h = O.hadamard_matrix(g, tag).astype(np.float64)
            acc = (x.astype(np.float64).reshape(37, 3, g) @ h).reshape(37, 3 * g)
            once = acc.astype(np.float32) if tag == "f32" else _round_once(acc, tag).astype(np.float32)
            assert np.array_equal(once, want), (g, tag, amp, "one rounding of the exact product")


def test_generator_rows():
    for tag in H.TAGS:
        x = H.exact_rows(7, 1024, tag, 3, None, 256)
        ints, unit = H.split_rows(x)
        assert np.abs(ints).max() <= H.LIMIT[tag] and not ints[1].any() and ints[0].any()
        assert unit[0, 0] == 2.0 ** H.ROW_EXP[tag][0] and unit[3, 0] == 2.0 ** H.ROW_EXP[tag][1] and unit[4, 0] == 1.0
        rot = np.abs(H.expected_rotation(x, 256, tag)[2])
        assert (rot == rot.max()).sum() == 1 and rot.max() == 16.0 * H.LIMIT[tag]  # amp g c = amp sqrt(g)
        # the tiny row's scale leaves RowDiv::fast's exponent window (biased exponent in (67, 187)) in bf16 / f32
        if tag != "f16":
            s = O.rowquant(H.expected_rotation(x, 256, tag), "int8")[1][0]
            assert ((int(np.float32(s).view(np.uint32)) >> 23) & 0xff) <= 127 - 60
    p = H.exact_rows(5, 640, "bf16", 3)  # no rotation: a single dominant element
    assert np.abs(p[2]).max() == 256 and np.sort(np.abs(p[2]))[-2] <= 8


def test_case_tables_name_every_reachable_form():
    named = H.all_case_forms()
    for form, m, k in H.HAD256_CASES:
        assert {H.rowquant_form(m, k, tag, 256) for tag in ("bf16", "f16")} == {form}
    for form, m, k, pf in H.ROWQUANT_CASES:
        got = {H.rowquant_form(m, k, tag, g, mode == "asym", False, pf) for tag, g, mode in H.fwht_configs(m, k, pf)}
        assert got == {"fwht-" + form}, (form, k, got)
        assert {H.rowquant_form(m, k, tag, 0, False, False, pf) for tag in H.TAGS} == {"plain-" + form}
    # every group meets every dtype and every quantizer mode somewhere in table (c)
    met = {cfg for _, m, k, pf in H.ROWQUANT_CASES for cfg in H.fwht_configs(m, k, pf)}
    for g in H.GROUPS:
        for tag in H.TAGS:
            assert any((tag, g, mode) in met for mode in ("int8", "fp8", "asym")), (g, tag)
        assert {mode for t, gg, mode in met if gg == g} == {"int8", "fp8", "asym"}, g
    # the dispatcher over a grid of every class of its inputs: each 256-column step up to 20480 and 8 columns beside every 512
    ks = sorted({j * 256 for j in range(1, 81)} | {j * 512 + d for j in range(1, 40) for d in (-8, 8)})
    seen = set()
    for k in ks:
        for m in (1, 3, 5, 1024, 1025, 2048, 2049, 5000):
            for tag in H.TAGS:
                for g in (0,) + tuple(g for g in (8, 256, 512) if k % g == 0):
                    for asym in (False, True):
                        for pf in (False, True):
                            seen.add(H.rowquant_form(m, k, tag, g, asym, False, pf))
                        if tag != "f32":
                            seen.add(H.rowquant_form(m, k, tag, g, asym, True))
    assert seen == named, (sorted(seen - named), sorted(named - seen))


def test_tuning_variables_are_refused(monkeypatch):
    for var in H.TUNING_ENV:
        monkeypatch.setenv(var, "1")
        with pytest.raises(AssertionError):
            H.rowquant_form(5, 768, "bf16", 256)
        monkeypatch.delenv(var)
    assert H.rowquant_form(5, 768, "bf16", 256) == "had256-NG4-W1"


# ------------------------------------------------------------------------------------------------
# a numpy model of the kernels' rotation, with one fault at a time
# ------------------------------------------------------------------------------------------------
def butterflies(ints: np.ndarray, g: int, flip=None) -> np.ndarray:
    """Integer sums by the kernels' butterflies (hadamard_dev.h): power-of-4 groups digit by digit, y(i) = S - 2 x(3 - i); the others bit by
    bit, (a + b, a - b).  flip = (stage, position): that stage computes S + 2 x(3 - i) / b - a at that one digit value / the high half."""
    m, k = ints.shape
    x = ints.reshape(m * (k // g), g).astype(np.int64)
    radix = 4 if H.is_pow4(g) else 2
    nd = int(round(np.log(g) / np.log(radix)))
    x = x.reshape((-1,) + (radix,) * nd)
    for d in range(nd):
        ax = nd - d  # digit d: the last axis is the lowest digit
        if radix == 4:
            s = x.sum(axis=ax, keepdims=True)
            y = s - 2 * np.flip(x, axis=ax)
            if flip is not None and flip[0] == d:
                idx = [slice(None)] * x.ndim
                idx[ax] = flip[1]
                y[tuple(idx)] = (s + 2 * np.flip(x, axis=ax))[tuple(idx)]
        else:
            a, b = np.take(x, 0, axis=ax), np.take(x, 1, axis=ax)
            hi = (b - a) if (flip is not None and flip[0] == d) else (a - b)
            y = np.stack([a + b, hi], axis=ax)
        x = y
    return x.reshape(m, k)


def model(x, g, tag, flip=None, c=None, round_first=False, transposed_group=None):
    ints, unit = H.split_rows(x)
    s = butterflies(ints, g, flip)
    if transposed_group is not None:  # a group of 256 as a 16 x 16 matrix with its two factors' index halves exchanged: element 16 r + c <-> 16 c + r
        assert g == 256
        lo = transposed_group * 256
        s[:, lo:lo + 256] = s[:, lo:lo + 256].reshape(-1, 16, 16).transpose(0, 2, 1).reshape(-1, 256)
    c = O.hadamard_scale(g, tag) if c is None else c
    if round_first:
        with np.errstate(under="ignore", over="ignore"):  # (float16: the unscaled sum may pass 65504 -- one more way this fault shows)
            s32 = O.round_dtype((s.astype(np.float64) * unit).astype(np.float32), tag)
            return O.round_dtype((s32 * np.float32(c)).astype(np.float32), tag)
    with np.errstate(over="ignore"):  # (a faulty float16 sum may pass 65504)
        return H.scaled_round(s, unit, c, tag)


@pytest.mark.parametrize("tag", H.TAGS)
@pytest.mark.parametrize("g", H.GROUPS)
def test_model_without_a_fault_is_exact_and_every_fault_shows(g, tag):
    x = H.exact_rows(5, 3 * g, tag, 2, None, g)
    want = H.expected_rotation(x, g, tag)
    assert _same(model(x, g, tag), want), "the butterfly model itself"
    radix = 4 if H.is_pow4(g) else 2
    stages = int(round(np.log(g) / np.log(radix)))
    for stage in range(stages):  # one partner sign, in every stage
        for pos in (range(4) if radix == 4 else (1,)):
            assert not _same(model(x, g, tag, flip=(stage, pos)), want), ("partner sign", stage, pos)
    if tag == "bf16":  # the scale constant one bf16 ulp up / down
        c = np.float32(O.hadamard_scale(g, tag))
        for off in (1 << 16, -(1 << 16)):  # (bf16 keeps the high 16 bits of the float32 pattern)
            c_off = float(np.uint32(int(c.view(np.uint32)) + off).view(np.float32))
            assert c_off != float(c) and not _same(model(x, g, tag, c=c_off), want), ("scale constant", off)
    # rounded to T before the scale instead of after: a different value only where the scale is no power of two (a power of two commutes
    # with a rounding) and the integer sum can leave T (never in float32)
    if not H.is_pow4(g) and tag != "f32":
        assert not _same(model(x, g, tag, round_first=True), want), "rounding before the scale"
    if g == 256:
        for grp in range(3):
            assert not _same(model(x, g, tag, transposed_group=grp), want), ("transposed factors", grp)


def test_one_hot_rows_expect_the_sign_matrix():
    for g in H.GROUPS:
        x = H.one_hot_rows(g, "f16", 2 * g)
        want = H.expected_rotation(x, g, "f16")
        v = x[np.arange(g), g + np.arange(g)]
        assert not want[:, :g].any()
        assert np.array_equal(np.sign(want[:, g:]), np.sign(v)[:, None] * H.sign_matrix(g))
