"""The column quantizer of the int8 training Linear (csrc/colquant.hip, sdnq_hip_colquant_t) at the sizes it was built for, and the
three products that run on its operands.  Every comparison is torch.equal on bits; the one bound is the project's grad_bias_bound on
random data (a float32 sum of thousands of terms has no order-free value).

What the shapes reach (train_linear_util.CENSUS_SHAPES / EDGE_SHAPES; tests/test_train_linear_host.py asserts each entry against
cq_plan, and cq_plan against the library's workspace size) -- the fixtures of tests/test_train_linear_gpu.py stop at one 128-row pass,
three slabs, two row tiles and C >= 48:

  3969 x 8       32 slabs of 128 rows, the last holds 1 row; 16 row tiles; one of the eight column lanes works
  4097 x 72      17 slabs of 256 (2 passes of the statistics loop), the last holds 1 row; 17 row tiles, the last holds 1 row; a partial
                 second column tile
  8200 x 24      22 slabs of 384 (3 passes), the last holds 136 rows; 33 row tiles
  4100 x 2056    33 column tiles, so the plan asks for 16 slabs: 11 of 384, the last holds 260 rows
  260 x 32712    512 column tiles, so the plan asks for 1 slab: 384 rows (3 passes, the third holds 4 rows)
  1280 x 16, 1536 x 208    the tie and exponent-range inputs: 10 and 12 slabs, 5 and 6 row tiles

Expected values: the census inputs carry their own (train_linear_util.exact_matrix: codes q, scales 2^e, integer column sums); the
edge inputs and the random chain come from the C oracle (oracle_colquant_t, oracle_chain), the exact-sum chain from float64 products
rounded once."""
import pytest
import torch

from tests import rowquant_inputs
from tests import train_linear_util as R

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _ops():
    from sdnq_amd import ops
    return ops


def _train():
    from sdnq_amd import training
    return training


def bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def bad_columns(q_t, s, ref_q, ref_s):
    """[(column, kernel scale, expected scale)] of the columns whose codes or scale differ."""
    bad = ((q_t.cpu() != ref_q).any(1) | (bits(s.cpu()) != bits(ref_s)).reshape(-1)).nonzero().reshape(-1).tolist()
    return [(c, float(s[c]), float(ref_s[c])) for c in bad[:8]]


# ---- a. census on constructed inputs ----------------------------------------------------------------------------------------------
# (the widest shape once, in bf16: the dtypes differ in the loads, which the other four shapes cover)
CENSUS_CASES = [(s, dt) for s in R.CENSUS_SHAPES for dt in DTYPES if s != (260, 32712) or dt == torch.bfloat16]


def case_id(v):
    return R.TAG[v] if isinstance(v, torch.dtype) else "x".join(map(str, v))


@pytest.mark.parametrize("shape,dtype", CENSUS_CASES, ids=case_id)
def test_census_of_rows_and_columns(shape, dtype, gpu_device):
    """Codes q, scales 2^e and integer column sums, known without any reference: each column's +-127 sits at row 0, at row R - 1 or in a
    later pass of some slab, so a row the statistics pass does not read changes that column's scale and every code in it, and every entry
    is non-zero, so a row read twice or not at all changes every column sum."""
    r, c = shape
    ops = _ops()
    x, q, e = R.exact_matrix(r, c, torch.Generator().manual_seed(r + c), None, R.census_pin_rows(r, c))
    xd = x.to(dtype).to(gpu_device)
    assert torch.equal(xd.float().cpu(), x)
    want_s = torch.exp2(e.float()).reshape(c, 1)
    want_sum = x.double().sum(0)
    q_t, s, colsum = ops.colquant_t(xd, want_colsum=True)
    assert q_t.shape == (c, (r + 15) // 16 * 16) and q_t.dtype == torch.int8
    wrong = (q_t[:, :r].cpu() != q.t())
    assert not wrong.any(), ("codes", int(wrong.sum()), "first (column, row)", wrong.nonzero()[:4].tolist())
    assert same_bits(s, want_s), ("scales", bad_columns(q_t[:, :r], s, q.t(), want_s))
    assert not q_t[:, r:].any(), "pad bytes"
    assert colsum.dtype == torch.float32 and torch.equal(colsum.double().cpu(), want_sum), \
        ("colsum", ((colsum.double().cpu() - want_sum) / torch.exp2(e.double())).abs().max())
    # a strided view (ldx > C) and a second call give the same bits
    wide = torch.cat([xd, torch.full_like(xd, 3.0)], 1)[:, :c]
    assert wide.stride(0) == 2 * c
    for again in (ops.colquant_t(wide, want_colsum=True), ops.colquant_t(xd, want_colsum=True)):
        assert torch.equal(again[0], q_t) and same_bits(again[1], s) and same_bits(again[2], colsum)
    if (r, c) == (4097, 72):
        # the C ABI with ld_t = 4608 = 18 row tiles: the last one is pad only; row C of the buffer is a guard
        from sdnq_amd import _lib
        lib = _lib.load()
        ld_t = 4608
        out = torch.full((c + 1, ld_t), 77, device=gpu_device, dtype=torch.int8)
        xs = torch.empty(c, device=gpu_device, dtype=torch.float32)
        nbytes = lib.sdnq_hip_colquant_t_workspace_bytes(r, c)
        ws = torch.empty(nbytes, device=gpu_device, dtype=torch.uint8)
        ops.check(lib.sdnq_hip_colquant_t(xd.data_ptr(), ops.float_code(dtype), r, c, xd.stride(0), out.data_ptr(), ld_t, xs.data_ptr(), None,
                                          ws.data_ptr(), nbytes, ops._stream(xd)), "colquant_t")
        assert torch.equal(out[:c, :r].cpu(), q.t()) and not out[:c, r:].any() and (out[c] == 77).all()
        assert same_bits(xs.reshape(c, 1), want_s)


# ---- b. ties and near-ties per column ---------------------------------------------------------------------------------------------
def test_rounding_ties_and_near_ties_per_column(gpu_device):
    """The ten rows of test_rowquant_rounding_ties_and_near_ties as ten columns (1280 x 16 with six zero columns): half to even on exact
    ties, and the right side of values one ulp beside a tie, in the column kernel's own fast branch."""
    x = torch.zeros(1280, 16)
    x[:, :10] = torch.from_numpy(rowquant_inputs.ties_and_near_ties()).t()
    ref_q, ref_s = R.oracle_colquant_t(x)
    q_t, s, _ = _ops().colquant_t(x.to(gpu_device))
    assert same_bits(q_t, ref_q) and same_bits(s, ref_s), bad_columns(q_t, s, ref_q, ref_s)
    assert not s[10:].any() and not q_t[10:].any()


# ---- c. the exponent range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: R.TAG[d])
def test_division_over_the_exponent_range_per_column(dtype, gpu_device):
    """The 207 rows of test_rowquant_division_shortcut_over_the_exponent_range as columns, plus a zero column (1536 x 208): columns on
    both sides of the 2^+-60 guard of RowDiv, subnormal scales and all-ones significands share waves with ordinary columns -- a wave of
    colquant_t_kernel runs its fast and its slow branch side by side, which a wave of the row quantizers never does."""
    x = torch.zeros(1536, 208)
    x[:, :207] = torch.from_numpy(rowquant_inputs.exponent_range()).t()
    x = x.to(dtype)
    ref_q, ref_s = R.oracle_colquant_t(x)
    q_t, s, _ = _ops().colquant_t(x.to(gpu_device))
    assert same_bits(q_t, ref_q) and same_bits(s, ref_s), ("(column, scale, expected scale)", bad_columns(q_t, s, ref_q, ref_s))
    assert s[207] == 0 and not q_t[207].any()


# ---- d. the non-finite convention ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: R.TAG[d])
def test_non_finite_columns_follow_the_row_quantizer(dtype, gpu_device):
    """colquant.hip documents sdnq_hip_rowquant's convention for NaN and inf: exactly that, per column, and the oracle's bits on every
    column that is finite throughout.  (The inf element of an inf column -- the quotient inf / inf -- leaves the row quantizer as -128;
    the column kernel used to flush it to 0.)"""
    ops = _ops()
    r, c = 530, 40
    x = torch.randn(r, c, generator=torch.Generator().manual_seed(40)).to(dtype)
    x[17, 3], x[300, 12], x[529, 21] = float("nan"), float("inf"), float("-inf")
    x[:, 30] = 0
    finite = torch.isfinite(x).all(0)
    assert int(finite.sum()) == c - 3
    xd = x.to(gpu_device)
    q_t, s, _ = ops.colquant_t(xd)
    # (sdnq_hip_rowquant takes rows of a multiple of 8 elements: x^T with six zero columns, which change neither a row's amax nor the
    # codes in front of them)
    xt = torch.zeros(c, 536, device=gpu_device, dtype=dtype)
    xt[:, :r] = xd.t()
    rq, rs, _, _ = ops.rowquant(xt, ops.MM_I8)
    assert not rq[:, r:].any()
    rq = rq[:, :r]
    assert same_bits(q_t[:, :r], rq) and same_bits(s, rs.reshape(c, 1)), bad_columns(q_t[:, :r], s, rq.cpu(), rs.reshape(c, 1).cpu())
    assert not q_t[:, r:].any()
    ref_q, ref_s = R.oracle_colquant_t(x)
    assert same_bits(q_t[finite.to(gpu_device)], ref_q[finite]) and same_bits(s[finite.to(gpu_device)], ref_s[finite])
    assert s[30] == 0 and not q_t[30].any()


# ---- e. the three products at training size against the oracle chain ----------------------------------------------------------------
def chain_inputs(m, n, k, dtype, seed):
    """randn x [M][K], W [N][K], bias [N], dY [M][N] with an all-zero token row (x and dY), an all-zero input channel (x and W), and a row
    of rounding ties in each of x, W and dY (quotients k + 0.5 at a power-of-two scale near the data's magnitude; every value is a bf16
    and a float16 number)."""
    g = torch.Generator().manual_seed(seed)
    x, w, dy = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * 0.05, torch.randn(m, n, generator=g) * 0.3
    bias = torch.randn(n, generator=g)
    for t, e in ((x, -5), (w, -11), (dy, -7)):
        width = t.shape[1]
        t[5] = (torch.randint(-126, 126, (width,), generator=g) + 0.5) * 2.0 ** e
        t[5, width - 1] = 127.0 * 2.0 ** e
    x[m // 2], dy[m // 2] = 0, 0
    x[:, 3], w[:, 3] = 0, 0
    return x.to(dtype), w.to(dtype), bias.to(dtype), dy.to(dtype)


CHAIN_CASES = [(s, dt) for s in ((4097, 80, 144), (8200, 48, 32), (520, 1104, 528), (33, 16, 16)) for dt in DTYPES
               if dt != torch.float32 or s == (4097, 80, 144)]


def run(fn, x, w, bias, dy):
    x, w, bias = (t.detach().clone().requires_grad_(True) for t in (x, w, bias))
    y = fn(x, w, bias)
    y.backward(dy)
    return y.detach(), x.grad, w.grad, bias.grad


@pytest.mark.parametrize("shape,dtype", CHAIN_CASES, ids=case_id)
def test_products_bit_equal_to_the_oracle_chain(shape, dtype, gpu_device):
    """y, grad_input and grad_weight of both autograd functions against oracle.rowquant + oracle.scaled_mm: M' = 4112 and 8208 are long
    reductions that are no multiple of the 256-row tile, (33, 16, 16) is the smallest problem the route takes."""
    T = _train()
    m, n, k = shape
    host = chain_inputs(m, n, k, dtype, m + n + k)
    x, w, bias, dy = host
    want = R.oracle_chain(x, w, bias, dy, dtype)
    total, bound = R.grad_bias_bound(dy, dtype)
    dev = [t.to(gpu_device) for t in host]
    for fn in (T.int8_matmul_dynamic_with_backward, T.int8_matmul_dynamic_with_backward_ckpt):
        got = run(fn, *dev)
        for name, g, ref in zip(("y", "grad_input", "grad_weight"), got, want):
            assert g.dtype == dtype and g.shape == ref.shape
            diff = bits(g.cpu()) != bits(ref)
            assert not diff.any(), (fn.__self__.__name__, name, int(diff.sum()), "of", diff.numel(), "first", diff.nonzero()[:4].tolist())
        err = (got[3].double().cpu() - total).abs()
        print(shape, R.TAG[dtype], "grad_bias err / bound", float((err / bound).max()))
        assert got[3].dtype == dtype and (err <= bound).all(), (fn.__self__.__name__, "grad_bias")


# ---- f. exact sums for the same chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: R.TAG[d])
@pytest.mark.parametrize("shape", [(4097, 80, 144), (520, 1104, 528)], ids=case_id)
def test_products_of_exact_operands_are_the_float64_products_rounded_once(shape, dtype, gpu_device):
    """Operands q * 2^e with a +-127 in every row and every column: every row scale and column scale is 2^e, every code is q, every
    accumulator is an integer below 2^24, so each output is the float64 product (plus the bias, an integer times 2^-7 like x . W^T)
    rounded once to the dtype, and grad_bias the exact column sum rounded once.  No reference kernel is involved."""
    T = _train()
    m, n, k = shape
    g = torch.Generator().manual_seed(m + n + k)
    (x, xq), (w, wq), (dy, gq) = R.exact_operand(m, k, g, -2), R.exact_operand(n, k, g, -5), R.exact_operand(m, n, g, -1)
    bias = torch.randint(-64, 65, (n,), generator=g).float() * 2.0 ** -7
    acc = (xq.double() @ wq.double().t() + bias.double() * 2.0 ** 7, gq.double() @ wq.double(), gq.double().t() @ xq.double(), gq.double().sum(0))
    exact = [a * s for a, s in zip(acc, (2.0 ** -7, 2.0 ** -6, 2.0 ** -3, 2.0 ** -1))]
    assert torch.equal(exact[0], x.double() @ w.double().t() + bias.double()) and torch.equal(exact[2], dy.double().t() @ x.double())
    print(shape, "max |acc|", [float(a.abs().max()) for a in acc])
    for a, v in zip(acc, exact):
        assert a.abs().max() < 2 ** 24 and torch.equal(v.float().double(), v)   # float32 holds each exactly: the cast below rounds once
        assert torch.isfinite(v.to(dtype)).all()
    want = [v.to(dtype) for v in exact]
    dev = [t.to(dtype).to(gpu_device) for t in (x, w, bias, dy)]
    for t, ref in zip(dev, (x, w, bias, dy)):
        assert torch.equal(t.float().cpu(), ref)
    for fn in (T.int8_matmul_dynamic_with_backward, T.int8_matmul_dynamic_with_backward_ckpt):
        got = run(fn, *dev)
        for name, gt, ref in zip(("y", "grad_input", "grad_weight", "grad_bias"), got, want):
            assert gt.dtype == dtype and gt.shape == ref.shape
            diff = bits(gt.cpu()) != bits(ref)
            assert not diff.any(), (fn.__self__.__name__, name, int(diff.sum()), "of", diff.numel(), "first", diff.nonzero()[:4].tolist())
