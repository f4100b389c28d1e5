"""CPU checks of the few-row census (tests/skinny_util.py): the case table reaches every launcher path and every loop boundary, every planted
case is inside the exact-arithmetic budget, the float64 expectation is the pinned oracle's, and the exact-sum check can see a one-code, a
swapped-column and a lost-tail fault in every case.  Nothing here runs a kernel."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import skinny_util as S

KERNELS = ("generic", "fast", "had256", "svd", "svd32")


def test_every_launch_path_is_reached():
    reached = {c.path for c in S.CASES}
    assert reached == set(S.ALL_PATHS), (sorted(set(S.ALL_PATHS) - reached), sorted(reached - set(S.ALL_PATHS)))
    for c in S.CASES:  # every case runs on the kernel it is laid out for
        assert c.path.split("-")[0] == c.kernel, (c.id, c.path)


def test_every_cell_meets_every_k_class():
    """kernel x code width x MROWS bucket x T at each K class of the kernel."""
    seen = {(c.path, c.tag, c.k) for c in S.CASES}
    for kernel, tags in (("generic", ("bf16", "f16", "f32")), ("fast", ("bf16", "f16", "f32")), ("had256", ("bf16", "f16")), ("svd", ("bf16", "f16")),
                         ("svd32", ("bf16", "f16"))):
        for path in (p for p in S.ALL_PATHS if p.split("-")[0] == kernel):
            key = kernel if kernel != "svd32" else f"svd32-{path.split('-')[1][0]}"
            for k in S.K_CLASSES[key]:
                for tag in tags:
                    assert (path, tag, k) in seen, (path, tag, k)


@pytest.mark.parametrize("key", sorted(S.K_CLASSES))
def test_k_classes_straddle_the_loop_period(key):
    """A K below one trip of the kernel's loop, one that ends on a trip, and one that starts another trip with at most one block (had256: one
    256-group; 4-bit svd32, K % 64 == 0: two blocks)."""
    kernel = key.split("-")[0]
    period = S.PERIOD[kernel]
    just = {"generic": 16, "fast": 16, "had256": 256, "svd": 32, "svd32": 64 if key.endswith("4") else 32}[kernel]
    ks = S.K_CLASSES[key]
    assert any(k < period for k in ks), (key, "below")
    assert any(k % period == 0 for k in ks), (key, "at")
    assert any(k > period and 0 < k % period <= just for k in ks), (key, "just above")
    if kernel == "svd32":  # the ring of four stages: a slot is read again after its refill from K = 640 on
        assert any(k < 640 for k in ks) and any(k == 640 for k in ks) and any(k > 640 for k in ks)


def test_rank_32_with_many_groups_leaves_the_dma_kernel():
    c = next(c for c in S.CASES if c.rank == 32 and c.gs == 16)
    assert c.k // c.gs > 64 and c.path == "svd-8bit-MR2"
    assert all(c.path.startswith("svd-") for c in S.CASES if c.rank == 32 and c.x_align == 8)
    assert any(c.rank == 32 and c.k // c.group > 1 and c.path.startswith("svd32") and S.plant(c).zp is not None for c in S.CASES)


def test_extras_are_in_the_table():
    for kernel in KERNELS:
        mine = S.cases_of(kernel)
        assert any(c.strided for c in mine) and any(not c.bias for c in mine) and any(c.repeat == 3 for c in mine), kernel
    gen = S.cases_of("generic")
    for wdt in ("int3", "int5", "uint7", "uint2", "float6_e3m2fn", "fp8"):
        assert any(c.wdt == wdt for c in gen), wdt
    assert any(c.codebook for c in gen) and any(c.scale_tag != "f32" and c.scale_tag != c.tag for c in gen)
    assert any(not c.bias and c.m == 32 for c in gen)
    assert {c.had for c in gen if c.had} == {16, 64, 256} and {c.had for c in S.cases_of("fast") if c.had} >= {16, 64, 256}
    assert any(c.had == 256 and c.tag == "f32" and c.path.startswith("fast") for c in S.CASES)


@pytest.mark.parametrize("kernel", KERNELS)
def test_planted_invariants_and_oracle_tie(kernel):
    """plant() asserts representability, the span budget and normal numbers; the float64 expectation equals the oracle's dequantize and
    linear_float on the same layer bit for bit (both are exact)."""
    for c in S.cases_of(kernel):
        p = S.plant(c)
        S.check_invariants(p)
        assert p.span_bits <= S.BUDGET_BITS
        wo = S.oracle_weight(p)
        assert np.array_equal(wo.astype(np.float64), p.w), (c.id, "planted weight vs the oracle's dequantize", S.first_mismatch(wo.astype(np.float64), p.w))
        want = p.expected()
        got = O.linear_float(p.x.astype(np.float32), wo, None if p.bias is None else p.bias.astype(np.float32), c.tag)
        assert np.array_equal(O.to_bits(got, c.tag), O.to_bits(want, c.tag)), (c.id, "expectation vs oracle.linear_float", S.first_mismatch(got, want))


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_sum_check_sees_planted_faults(kernel):
    for c in S.cases_of(kernel):
        p = S.plant(c)
        want = O.to_bits(p.expected(), c.tag)
        for name, edit in S.EDITS.items():
            w = edit(p)
            assert not np.array_equal(w, p.w), (c.id, name, "the edit changed nothing")
            acc = p.x @ w.T + (0.0 if p.bias is None else p.bias[None, :])
            got = O.to_bits(O.round_dtype(acc.astype(np.float32), c.tag), c.tag)
            assert not np.array_equal(got, want), (c.id, name, "no expected output bit changes")


@pytest.mark.parametrize("kernel", KERNELS)
def test_boundary_columns_cover_every_block_edge(kernel):
    for k in sorted({c.k for c in S.cases_of(kernel)}):
        cols = set(S.boundary_columns(kernel, k).tolist())
        for step in (S.BLOCK[kernel], S.PERIOD[kernel]):
            for b0 in range(0, k, step):
                assert b0 in cols and min(b0 + step, k) - 1 in cols
        assert {0, k - 16, k - 1} <= cols and max(cols) < k


def test_tie_cases_tell_one_rounding_from_two():
    """The zero-point tie layers: the oracle (fma rounded to float32, then to T) and a single rounding of the exact q s + z give other weights at
    a large part of the elements, on every kernel that takes zero points."""
    assert {c.kernel for c in S.TIE_CASES} == {"generic", "fast", "svd", "svd32"}
    for c in S.TIE_CASES:
        assert c.path.split("-")[0] == c.kernel, (c.id, c.path)
        p = S.plant_tie(c)
        assert S.representable(p.w, c.tag) and S.all_normal(p.w, c.tag)
        assert (p.w != p.w_stored).mean() > 0.2, (c.id, float((p.w != p.w_stored).mean()))
