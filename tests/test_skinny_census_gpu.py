"""The few-row linear kernels (sdnq_amd/csrc/skinny.hip) per launch path, called through ops.linear_skinny / ops.linear_skinny_svd.

  * exact sums: on the planted cases of tests/skinny_util.py every output must carry the bits of round_T(float64 sum + bias) -- nothing can
    round before the output does, whatever the order of the additions;
  * column census: one-hot activation rows read back the weight element the kernel formed for every (n, k): all K columns for the largest
    MROWS bucket of each (kernel, code width, T), the boundary columns of every pass / chunk / group / block for the others;
  * the same census on weights quantized from Gaussian weights (arbitrary scales) against the oracle's dequantized weight: bit-equal for the
    plain formats, within 1 ulp of T (the contract in the header of tests/test_gpu_parity.py) for SVD and Hadamard layers, or within the
    distance of the unfused dequantize kernel to the oracle at the same element where that is larger;
  * routing: SDNQLinear with FUSED_SKINNY reaches the same bits as the direct call.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import skinny_util as S
from tests.modules_util import oracle_from_module, to_f32_numpy

pytestmark = pytest.mark.gpu

from sdnq_amd import ops  # noqa: E402

KERNELS = ("generic", "fast", "had256", "svd", "svd32")


def _bits(t: torch.Tensor, tag: str) -> np.ndarray:
    return O.to_bits(t.detach().float().cpu().numpy(), tag)


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_sums_per_launch_path(kernel, gpu_device):
    S.require_default_tuning()
    failures = []
    cases = S.cases_of(kernel)
    for c in cases:
        p = S.plant(c)
        qw, down_t = S.device_weight(p, gpu_device)
        x = S.device_x(p.x, c, gpu_device)
        bias = None if p.bias is None else torch.from_numpy(p.bias.astype(np.float32)).to(S.TAG_DT[c.tag]).to(gpu_device)
        outs = [S.run(c, qw, down_t, x, bias) for _ in range(c.repeat)]
        want = O.to_bits(p.expected(), c.tag)
        got = [_bits(y, c.tag) for y in outs]
        if any(not np.array_equal(g, got[0]) for g in got[1:]):
            failures.append((c.id, c.path, "the same call gave other bits"))
        bad, first = S.first_mismatch(got[0], want)
        if bad:
            m, n = first
            failures.append((c.id, c.path, f"{bad} of {want.size} outputs differ, first at (m, n) = {first}: got {float(outs[0][m, n]):.9g}, "
                                           f"want {float(p.expected()[m, n]):.9g}"))
    print(f"skinny exact sums: {kernel}: {len(cases)} cases, {len(failures)} failed")
    assert not failures, (len(failures), failures[:12])


def _census_cases(kernel):
    """Per (path, T) of the kernel the plain main-table case with the largest K (and M): [(case, all columns?)]: all K columns for the largest
    MROWS bucket of each (kernel, code width, T), the boundary set for the others."""
    best = {}
    for c in S.cases_of(kernel):
        if c.strided or c.x_align != 16 or c.repeat > 1 or c.note or not c.bias:
            continue
        key = (c.path, c.tag)
        if key not in best or (c.k, c.m) > (best[key].k, best[key].m):
            best[key] = c
    top = {}
    for (path, tag), c in best.items():
        cell = (path.rsplit("-", 1)[0], tag)
        top[cell] = max(top.get(cell, 0), int(path.rsplit("MR", 1)[1]))
    return [(c, int(path.rsplit("MR", 1)[1]) == top[(path.rsplit("-", 1)[0], tag)]) for (path, tag), c in sorted(best.items())]


@pytest.mark.parametrize("kernel", KERNELS)
def test_column_census_on_planted_weights(kernel, gpu_device):
    S.require_default_tuning()
    failures = []
    picked = _census_cases(kernel)
    assert picked
    for c, full in picked:
        p = S.plant(c)
        qw, down_t = S.device_weight(p, gpu_device)
        cols = np.arange(c.k) if full else S.boundary_columns(kernel, c.k)
        got = S.census(c, qw, down_t, cols, gpu_device)
        want = p.w[:, cols].astype(np.float32)
        bad, first = S.first_mismatch(got, want)  # float ==: +0 and -0 agree
        if bad:
            n, j = first
            failures.append((c.id, c.path, f"{bad} of {want.size} weight elements differ, first at (n, k) = ({n}, {int(cols[j])}): got {got[n, j]:.9g}, "
                                           f"want {want[n, j]:.9g}"))
    print(f"skinny census (planted): {kernel}: {len(picked)} sweeps ({sum(f for _, f in picked)} over all K columns), {len(failures)} failed")
    assert not failures, (len(failures), failures[:12])


# (kernel, weights_dtype, group_size, T, M, K, N, Hadamard group, SVD rank)
REAL = [
    ("fast", "int8", -1, "bf16", 4, 4112, 70, 0, 0), ("fast", "uint8", -1, "f16", 2, 1040, 70, 0, 0), ("fast", "int4", 16, "f32", 4, 4112, 70, 0, 0),
    ("fast", "uint4", 16, "bf16", 1, 5136, 70, 0, 0),
    ("generic", "int5", -1, "bf16", 8, 2064, 70, 0, 0), ("generic", "uint7", 128, "f16", 3, 1152, 70, 0, 0), ("generic", "float6_e3m2fn", 32, "f32", 2, 1152, 70, 0, 0),
    ("generic", "int8", -1, "f32", 32, 1040, 70, 0, 0),
    ("had256", "int4", 64, "bf16", 4, 4352, 24, 256, 0), ("had256", "uint8", -1, "f16", 2, 4352, 24, 256, 0),
    ("fast", "int8", -1, "bf16", 4, 1280, 70, 16, 0), ("fast", "int4", 64, "f16", 2, 1280, 70, 64, 0), ("fast", "uint4", 32, "bf16", 3, 1280, 70, 32, 0),
    ("fast", "int8", -1, "f16", 4, 1280, 70, 128, 0), ("generic", "int8", -1, "bf16", 5, 1280, 70, 128, 0), ("generic", "int6", 32, "f16", 2, 1280, 70, 32, 0),
    ("svd", "int8", -1, "bf16", 3, 672, 72, 0, 16), ("svd", "uint4", 32, "f16", 2, 672, 72, 0, 48),
    ("svd32", "int8", -1, "bf16", 4, 1056, 72, 0, 32), ("svd32", "uint4", 64, "f16", 2, 1088, 72, 0, 32), ("svd32", "uint8", -1, "f16", 1, 640, 72, 0, 32),
]


MAX_LAUNCHES = 1300  # of one census: K = 5136 at M = 4 is 1284
ROUTING = [next(r for r in REAL if r[0] == kernel) for kernel in KERNELS]  # one layer per kernel


def _quantized_module(wdt, gs, tag, k, n, had, rank, device, bias=False):
    import sdnq_amd
    torch.manual_seed(k + n + had + rank)
    dt = S.TAG_DT[tag]
    lin = torch.nn.Linear(k, n, bias=bias).to(dt).to(device)
    cfg = sdnq_amd.SDNQConfig(weights_dtype=wdt, group_size=gs, use_quantized_matmul=False, use_svd=bool(rank), svd_rank=rank or 32,
                              use_hadamard=bool(had), hadamard_group_size=had or 256)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, cfg)
    dq = mod.sdnq_dequantizer
    assert bool(dq.use_hadamard) == bool(had) and (not had or dq.hadamard_group_size == had), (dq.use_hadamard, dq.hadamard_group_size)
    assert (getattr(mod, "svd_up", None) is not None) == bool(rank)
    return mod


def _ulp(ref: np.ndarray, tag: str) -> np.ndarray:
    mant, emin = {"bf16": (7, -126), "f16": (10, -14), "f32": (23, -126)}[tag]
    e = np.floor(np.log2(np.maximum(np.abs(ref.astype(np.float64)), 2.0 ** emin)))
    return np.exp2(e - mant)


@pytest.mark.parametrize("kernel,wdt,gs,tag,m,k,n,had,rank", REAL, ids=lambda v: str(v))
def test_column_census_on_quantized_weights(kernel, wdt, gs, tag, m, k, n, had, rank, gpu_device):
    from sdnq_amd import linear as L
    S.require_default_tuning()
    mod = _quantized_module(wdt, gs, tag, k, n, had, rank, gpu_device)
    dq = mod.sdnq_dequantizer
    st = L._state(mod)
    group = dq.group_size if dq.group_size > 0 else k
    path = S.launch_path(wdt, group, "f32", had, tag, m, k, rank)
    assert path.split("-")[0] == kernel, path
    case = S.Case(kernel, wdt, group, tag, m, k, had=had, rank=rank)
    down_t = st.svd_down.t().contiguous() if rank else None
    # all K columns up to MAX_LAUNCHES launches of the layer's own M rows, the boundary set of every pass / chunk / group / block beyond
    cols = np.arange(k) if -(-k // m) <= MAX_LAUNCHES else S.boundary_columns(kernel, k)
    got = S.census(case, st.qw, down_t, cols, gpu_device)
    ref = oracle_from_module(mod).dequantize(tag)[:, cols]
    assert got.shape == ref.shape == (n, len(cols))
    if not had and not rank:
        bad, first = S.first_mismatch(got, ref)
        assert not bad, (path, f"{bad} of {ref.size} weight elements differ from the oracle, first at (n, column index) = {first}")
        return
    ulp = _ulp(ref, tag)
    dist = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp
    unfused = to_f32_numpy(ops.dequant(st.qw, S.TAG_DT[tag], had))[:, cols]
    dist_unfused = np.abs(unfused.astype(np.float64) - ref.astype(np.float64)) / ulp
    worst = np.unravel_index(int(np.argmax(dist)), dist.shape)
    print(f"skinny census (quantized): {path} {wdt} g{gs} {tag} K={k} had={had} rank={rank}: fused max {dist.max():.3f} ulp "
          f"({int((dist > 0).sum())} of {dist.size} differ), unfused dequantize max {dist_unfused.max():.3f} ulp ({int((dist_unfused > 0).sum())} differ)")
    # per element: 1 ulp, or the unfused kernel's own distance at THAT element where it is larger (an element the oracle cancels to 0 has the
    # smallest subnormal as its ulp)
    over = dist > np.maximum(1.0, dist_unfused)
    assert not over.any(), (path, f"{int(over.sum())} of {dist.size} elements beyond max(1 ulp, unfused distance)", "worst", float(dist.max()),
                            "at (n, k)", (int(worst[0]), int(cols[worst[1]])), "fused", float(got[worst]), "unfused", float(unfused[worst]),
                            "oracle", float(ref[worst]))


@pytest.mark.parametrize("kernel,wdt,gs,tag,m,k,n,had,rank", ROUTING, ids=lambda v: str(v))
def test_module_routing_reaches_the_same_bits(kernel, wdt, gs, tag, m, k, n, had, rank, gpu_device):
    from sdnq_amd import linear as L
    assert L.FUSED_SKINNY
    mod = _quantized_module(wdt, gs, tag, k, n, had, rank, gpu_device, bias=True)
    st = L._state(mod)
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(S.TAG_DT[tag]).to(gpu_device)
    y_mod = mod(x)
    case = S.Case(kernel, wdt, gs if gs > 0 else k, tag, m, k, had=had, rank=rank)
    assert case.path.split("-")[0] == kernel
    y_direct = S.run(case, st.qw, st.svd_down.t().contiguous() if rank else None, x, mod.bias)
    assert np.array_equal(_bits(y_mod, tag), _bits(y_direct, tag)), (case.path, "module forward and direct call differ")


def test_zero_point_weights_round_to_float32_first(gpu_device):
    """Zero-point layers whose fma(q, s, z) lands on a tie of T once it is rounded to float32 (skinny_util.plant_tie): the weight every kernel
    forms must be the oracle's -- float32 first, then T -- at every element; one fused fma-and-convert rounds once and misses a fifth of them."""
    failures = []
    for c in S.TIE_CASES:
        p = S.plant_tie(c)
        qw, down_t = S.device_weight(p, gpu_device)
        got = S.census(c, qw, down_t, np.arange(c.k), gpu_device)
        bad, first = S.first_mismatch(got, p.w.astype(np.float32))
        if bad:
            once = int((got == p.w_stored.astype(np.float32)).sum())
            failures.append((c.id, c.path, f"{bad} of {got.size} weight elements differ from the oracle, first at (n, k) = {first}; "
                                           f"{once} equal the single rounding of the exact q s + z"))
    print(f"skinny census (ties): {len(S.TIE_CASES)} layers, {len(failures)} failed")
    assert not failures, failures
