"""Bit-exact tests of the DoRA kernels on the GPU: sdnq_hip_dora_normsq from the stored codes of every storage-format bucket and its
dense form, a row / column census of the norm kernel, sdnq_hip_lowrank_add_dora against sdnq_hip_lowrank_add and against the float32
restatement of its epilogue, and sdnq_hip_dora_bwd.  Inputs and expected values: tests/dora_util.py (exact-sum operands, the exactness
asserted on the CPU)."""
import numpy as np
import pytest
import torch

from sdnq_amd import ops
from tests import dora_util as D
from tests import lora_util as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# N: one full row tile plus a ragged one (N % 16 == 8), a single ragged tile, three tiles; K: one run, a ragged 64-column wave share,
# a ragged 256-column chunk, four chunks and a tail (the kernel has no other K boundary); rank: one chunk, a ragged 32-rank step, two
# steps, the largest
NORM_SHAPES = ((8, 16, 8), (24, 48, 24), (40, 208, 64), (24, 1040, 256), (40, 272, 8))


def _t(a: np.ndarray, tag: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(D.DT[tag]).to(DEV)


def _same(got: torch.Tensor, want: np.ndarray, what: str) -> None:
    g = got.float().cpu().numpy()
    bad = np.nonzero(g.view(np.uint32) != np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {g.size} differ, first at {tuple(int(b[0]) for b in bad)}: " \
                             f"got {g[tuple(b[0] for b in bad)]}, want {want[tuple(b[0] for b in bad)]}"


@pytest.mark.parametrize("fmt", D.FORMATS, ids=lambda f: f.id)
def test_normsq_from_codes_is_bit_exact(fmt):
    for i, (n, k, rank) in enumerate(NORM_SHAPES):
        if k % (fmt.group or k):
            k = -(-k // fmt.group) * fmt.group
            if k % 16:
                continue
        wt = D.plant_weight(fmt, n, k, seed=100 + i)
        qw = wt.device(DEV)
        w32 = ops.dequant(qw, torch.float32)
        _same(w32, wt.w.astype(np.float32), f"{fmt.id} {n}x{k}: the planted weight as sdnq_hip_dequant decodes it")
        _same(ops.dora_normsq(qw), D.normsq_expected(wt.w, None, None, D.SCALE, wt.er), f"{fmt.id} {n}x{k} without factors")
        up, down = D.plant_factors(n, k, rank, wt.er, seed=200 + i)
        want = D.normsq_expected(wt.w, up, down, D.SCALE, wt.er)
        for tag in ("bf16", "f16"):
            got = ops.dora_normsq(qw, _t(up, tag), _t(down, tag), D.SCALE)
            _same(got, want, f"{fmt.id} {n}x{k} rank {rank} {tag}")
            _same(ops.dora_normsq(qw, _t(up, tag), _t(down, tag), D.SCALE), got.cpu().numpy(), "a second call")


@pytest.mark.parametrize("tag", ("bf16", "f16"))
def test_normsq_dense_is_bit_exact(tag):
    for i, (n, k, rank) in enumerate(NORM_SHAPES):
        wt = D.plant_weight(D.Fmt("int8"), n, k, seed=300 + i)
        up, down = D.plant_factors(n, k, rank, wt.er, seed=400 + i)
        wide = torch.zeros((n, k + 24), dtype=D.DT[tag], device=DEV)
        wide[:, 8:8 + k] = _t(wt.w, tag)
        wd = wide[:, 8:8 + k]                                 # a column window of a wider buffer: ldw > k, 16-byte aligned rows
        _same(ops.dora_normsq_dense(wd), D.normsq_expected(wt.w, None, None, D.SCALE, wt.er), f"dense {n}x{k} without factors")
        _same(ops.dora_normsq_dense(wd, _t(up, tag), _t(down, tag), D.SCALE), D.normsq_expected(wt.w, up, down, D.SCALE, wt.er),
              f"dense {n}x{k} rank {rank}")


def test_norm_census_every_row_and_column_position():
    """One nonzero element at every (row of a 16-row tile and of the ragged tile behind it, column of a 256-column chunk and of the 16
    behind it) in turn: exactly that row's output is exactly its square."""
    n, k = 24, D.DN_KC + 16
    wd = torch.zeros((n, k), dtype=torch.bfloat16, device=DEV)
    outs, vals = [], []
    for row in range(n):
        for col in range(k):
            v = float(1 + (row * 7 + col) % 5)
            wd[row, col] = v
            outs.append(ops.dora_normsq_dense(wd))
            wd[row, col] = 0
            vals.append((row, v * v))
    got = torch.stack(outs).cpu().numpy()
    want = np.zeros_like(got)
    for i, (row, sq) in enumerate(vals):
        want[i, row] = sq
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f"{bad.size} planted positions give a wrong census, first (row, column) = {divmod(int(bad[0]), k)}"


def test_norm_census_with_factors():
    """The same through the matrix cores: up = one-hot rows, down = one nonzero: acc has ONE nonzero, at (row, column) -- every position in turn
    for the rank product alone (the weight is zero)."""
    n, k, rank = 24, D.DN_KC + 16, 40
    wd = torch.zeros((n, k), dtype=torch.bfloat16, device=DEV)
    up = torch.zeros((n, rank), dtype=torch.bfloat16, device=DEV)
    up[torch.arange(n), (torch.arange(n) * 3) % rank] = 2.0       # row r uses rank column 3 r % rank
    outs = []
    for col in range(k):
        down = torch.zeros((rank, k), dtype=torch.bfloat16, device=DEV)
        r = (col * 7) % rank
        down[r, col] = 3.0
        outs.append(ops.dora_normsq_dense(wd, up, down, D.SCALE))
    got = torch.stack(outs).cpu().numpy()
    want = np.zeros_like(got)
    for col in range(k):
        r = (col * 7) % rank
        for row in range(n):
            if (row * 3) % rank == r:
                want[col, row] = (D.SCALE * 2.0 * 3.0) ** 2
    assert np.array_equal(got, want), f"columns {np.nonzero((got != want).any(1))[0][:8]} give a wrong census"


# ---- lowrank_add_dora ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((33, 72, 16), (*L.ADD_TWO_TILES, 8)), ids=("one row tile per wave", "two row tiles per wave"))
def test_add_dora_with_c_one_is_lowrank_add_bf16_arbitrary_operands(shape):
    m, n, rank = shape
    assert L.add_row_tiles(m, n) == (2 if m > 1000 else 1)
    g = torch.Generator().manual_seed(m)
    t = torch.randn((m, rank), generator=g).to(torch.bfloat16).to(DEV)
    up = torch.randn((n, rank), generator=g).to(torch.bfloat16).to(DEV)
    up[::3] = 0                                                 # exactly zero sums: the element keeps its bits (a -0.0 included)
    y0 = torch.randn((m, n), generator=g).to(torch.bfloat16).to(DEV)
    y0[0, :8] = -0.0
    c = torch.ones(n, dtype=torch.float32, device=DEV)
    want = ops.lowrank_add(t, up, y0.clone(), 0.3)
    got = ops.lowrank_add_dora(t, up, y0.clone(), 0.3, c, None)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(DEV)  # with c == 1 the bias does not enter
    assert torch.equal(ops.lowrank_add_dora(t, up, y0.clone(), 0.3, c, bias).view(torch.int16), want.view(torch.int16))


def test_add_dora_with_c_one_is_lowrank_add_f16_exact_operands():
    m, n, rank = 33, 72, 16
    ex, y0, _ = L.add_case(m, n, rank, "f16")
    y = torch.from_numpy(y0).to(torch.float16).to(DEV)
    t, up = ex.a.to(DEV), ex.b.to(DEV)
    c = torch.ones(n, dtype=torch.float32, device=DEV)
    for scale in L.SCALES:
        want = ops.lowrank_add(t, up, y.clone(), scale)
        assert torch.equal(ops.lowrank_add_dora(t, up, y.clone(), scale, c, None).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("tag", ("bf16", "f16"))
@pytest.mark.parametrize("m", (1, 33, 257))
def test_add_dora_general_c_and_bias_equals_the_float32_restatement(m, tag):
    n, rank = 72, 40                                             # ragged N (no multiple of the 128-column tile), a ragged rank step
    ex, y0, _ = L.add_case(m, n, rank, tag)
    rng = np.random.default_rng(m)
    c = rng.uniform(0.25, 2.0, size=n).astype(np.float32)
    c[::7] = 1.0
    c[3] = 0.0
    bias = D.round_f32_to(rng.standard_normal(n).astype(np.float32) * 0.25, tag)
    z = D.round_f32_to(y0, tag)
    for b in (bias, None):
        want = D.add_dora_expected(ex.acc(), z, c, b, D.SCALE, tag)
        y = torch.from_numpy(z).to(D.DT[tag]).to(DEV)
        got = ops.lowrank_add_dora(ex.a.to(DEV), ex.b.to(DEV), y, D.SCALE, torch.from_numpy(c).to(DEV), None if b is None else _t(b, tag))
        _same(got, want, f"M = {m} {tag} bias {'on' if b is not None else 'off'}")


# ---- dora_bwd ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("bf16", "f16"))
def test_bwd_g_is_the_rounded_product_on_any_operands(tag):
    m, n = 300, 72
    g = torch.Generator().manual_seed(5)
    dy_dev = torch.randn((m, n + 8), generator=g).to(D.DT[tag]).to(DEV)[:, :n]   # rows of a wider buffer: lddy > n
    dy = dy_dev.cpu()
    y = torch.randn((m, n), generator=g).to(D.DT[tag])
    c = torch.rand(n, generator=g) * 2
    c[5] = 0.0
    got, q = ops.dora_bwd(dy_dev, y.to(DEV), None, c.to(DEV))
    want = D.bwd_g_expected(dy, c)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    g_only, none = ops.dora_bwd(dy_dev, None, None, c.to(DEV), want_q=False)
    assert none is None and torch.equal(g_only.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.isfinite(q).all()


@pytest.mark.parametrize("m", (1, D.DB_SLAB - 1, D.DB_SLAB, D.DB_SLAB + 1, 675))
def test_bwd_q_is_bit_exact_at_the_slab_edges(m):
    n = 72
    for tag in ("bf16", "f16"):
        for with_bias in (True, False):
            dy, y, b, want = D.bwd_case(m, n, tag, seed=m + (1 if with_bias else 0), with_bias=with_bias)
            c = torch.full((n,), 0.75, dtype=torch.float32, device=DEV)
            _, q = ops.dora_bwd(dy.to(DEV), y.to(DEV), None if b is None else b.to(DEV), c)
            _same(q, want, f"q at M = {m} {tag} bias {'on' if with_bias else 'off'}")
            _, q2 = ops.dora_bwd(dy.to(DEV), y.to(DEV), None if b is None else b.to(DEV), c)
            assert torch.equal(q.view(torch.int32), q2.view(torch.int32))
