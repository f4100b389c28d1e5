"""Int8 training Linear on the MI355X (sdnq_amd.training, csrc/colquant.hip) against the reference's fixtures (tests/golden/train_int8_*):
the column quantizer bit for bit, the three products against the GEMM on the fixture's own operands and against the reference within
the standing w8a8 bound, grad_bias, the two variants against each other, what the ckpt variant saves, needs_input_grad subsets, stream
capture and a small training loop.

Shapes: the fixtures' (tests/golden/make_golden_training.py) -- M = 33 / 72 (not multiples of 16), M = 300 (three 128-row statistics
slabs, two 256-row quantize tiles), C = 48 / 80 / 96 (partial 64-column tiles).  At these sizes the statistics loop of colstat_kernel
runs once per slab and at most three slabs meet; the sizes the kernel was built for -- several passes per slab, 32 slabs, tens of row
tiles, C = 8, hundreds of column tiles -- and the products against an independent oracle are in tests/test_colquant_exact_gpu.py."""
import pytest
import torch

from tests import train_linear_util as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = R.train_names()
_cache = {}


def fixture(name):
    """(meta, tensors on the CPU, tensors on the device), loaded once per name and never written to."""
    if name not in _cache:
        meta, t = R.load(name)
        _cache[name] = (meta, t, {k: v.to(DEV) for k, v in t.items()})
    return _cache[name]


def _ops():
    from sdnq_amd import ops
    return ops


def _train():
    from sdnq_amd import training
    return training


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def run(fn, d, need):
    x, w = d["x"].detach().clone().requires_grad_(need[0]), d["w"].detach().clone().requires_grad_(need[1])
    b = d["bias"].detach().clone().requires_grad_(need[2]) if "bias" in d else None
    y = fn(x, w, b)
    y.backward(d["dy"])
    return y.detach(), x.grad, w.grad, (b.grad if b is not None else None)


# the column-quantized operands: (source tensor, fixture codes as [R][C])
COL_OPERANDS = {"gi_w": ("w", lambda t: t["gi_w_q"]), "gw_x": ("x", lambda t: t["gw_x_q"]), "gw_dy": ("dy", lambda t: t["gw_dy_q"].t())}


@pytest.mark.parametrize("name", NAMES)
def test_colquant_t_bit_equal_to_the_reference(name):
    ops = _ops()
    meta, t, d = fixture(name)
    for key, (src, codes) in COL_OPERANDS.items():
        x2d = d[src].flatten(0, -2)
        r, c = x2d.shape
        q_t, s, colsum = ops.colquant_t(x2d, want_colsum=True)
        assert q_t.dtype == torch.int8 and q_t.shape == (c, (r + 15) // 16 * 16) and s.shape == (c, 1) and s.dtype == torch.float32
        assert torch.equal(q_t[:, :r].cpu(), codes(t).t()), (name, key, "codes")
        assert torch.equal(s.reshape(-1).cpu(), t[key + "_s"].reshape(-1)), (name, key, "scales")
        assert not q_t[:, r:].any(), (name, key, "pad bytes")
        # a strided view (ldx > C) gives the same bits; so does a second run (colsum has a fixed summation order)
        wide = torch.cat([x2d, torch.full_like(x2d, 3.0)], 1)[:, :c]
        assert wide.stride(0) == 2 * c
        for again in (ops.colquant_t(wide, want_colsum=True), ops.colquant_t(x2d, want_colsum=True)):
            assert torch.equal(again[0], q_t) and torch.equal(again[1], s) and torch.equal(again[2].view(torch.int32), colsum.view(torch.int32))
        total, bound = R.colsum_bound(t[src].flatten(0, -2))
        err = (colsum.double().cpu() - total).abs()
        print(name, key, "colsum err / bound", float((err / bound).max()))
        assert (err <= bound).all(), (name, key, "colsum")
        assert ops.colquant_t(x2d)[2] is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_colquant_t_zero_column_and_wide_pad(dtype):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(290, 72, generator=g).to(dtype)
    x[:, 5] = 0
    x[:, 70] = 0
    q_t, s, colsum = ops.colquant_t(x.to(DEV), want_colsum=True)
    rq, rs, rsum = R.colquant_t(x, want_colsum=True)
    assert torch.equal(q_t.cpu(), rq) and torch.equal(s.cpu(), rs)
    assert s[5] == 0 and s[70] == 0 and not q_t[5].any() and not q_t[70].any() and colsum[5] == 0
    # ld_t far beyond R through the C ABI: every byte of [R, ld_t) is zero and nothing past the buffer is touched
    from sdnq_amd import _lib
    lib = _lib.load()
    r, c, ld_t = 290, 72, 1024
    xd = x.to(DEV)
    out = torch.full((c + 1, ld_t), 77, device=DEV, dtype=torch.int8)
    xs = torch.empty(c, device=DEV, dtype=torch.float32)
    nbytes = lib.sdnq_hip_colquant_t_workspace_bytes(r, c)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    ops.check(lib.sdnq_hip_colquant_t(xd.data_ptr(), ops.float_code(dtype), r, c, xd.stride(0), out.data_ptr(), ld_t, xs.data_ptr(), None,
                                      ws.data_ptr(), nbytes, ops._stream(xd)), "colquant_t")
    assert torch.equal(out[:c, :r].cpu(), rq[:, :r]) and not out[:c, r:].any() and (out[c] == 77).all()
    assert torch.equal(xs.cpu(), rs.reshape(-1))


@pytest.mark.parametrize("name", NAMES)
def test_products_against_the_gemm_and_the_reference(name):
    """y, grad_input and grad_weight: bit-equal to ops.scaled_mm on the FIXTURE's codes and scales (the same kernel on bit-exact
    operands), and within the standing w8a8 bound of the reference's results (its CPU epilogue is addcmul, not an fma)."""
    ops, T = _ops(), _train()
    meta, t, d = fixture(name)
    need = tuple(meta["need"])
    dt = d["x"].dtype
    y, gi, gw, gb = run(T.int8_matmul_dynamic_with_backward, d, need)
    m, n, k = meta["M"], meta["N"], meta["K"]
    mp = (m + 15) // 16 * 16

    def padded(codes_cm):  # [C][M] codes -> [C][M'] with zero pad columns
        out = torch.zeros(codes_cm.shape[0], mp, device=DEV, dtype=torch.int8)
        out[:, :m] = codes_cm
        return out
    ref_y = ops.scaled_mm(ops.MM_I8, d["fwd_x_q"], d["fwd_w_q"].t().contiguous(), d["fwd_x_s"].reshape(-1), d["fwd_w_s"].reshape(-1),
                          d.get("bias"), dt)
    assert y.shape == t["y"].shape and y.dtype == dt
    assert torch.equal(bits(y.reshape(m, n)), bits(ref_y)), (name, "y vs the GEMM on the fixture's operands")
    R.assert_w8a8_close(y.cpu(), t["y"], (name, "y"))
    assert (gi is not None) == need[0] and (gw is not None) == need[1] and (gb is not None) == need[2]
    if need[0]:
        ref = ops.scaled_mm(ops.MM_I8, d["gi_dy_q"], d["gi_w_q"].t().contiguous(), d["gi_dy_s"].reshape(-1), d["gi_w_s"].reshape(-1), None, dt)
        assert gi.shape == t["x"].shape and torch.equal(bits(gi.reshape(m, k)), bits(ref)), (name, "grad_input vs the GEMM")
        R.assert_w8a8_close(gi.cpu(), t["grad_input"], (name, "grad_input"))
    if need[1]:
        ref = ops.scaled_mm(ops.MM_I8, padded(d["gw_dy_q"]), padded(d["gw_x_q"].t()), d["gw_dy_s"].reshape(-1), d["gw_x_s"].reshape(-1), None, dt)
        assert gw.shape == t["w"].shape and torch.equal(bits(gw), bits(ref)), (name, "grad_weight vs the GEMM")
        R.assert_w8a8_close(gw.cpu(), t["grad_weight"], (name, "grad_weight"))
    if need[2]:
        total, bound = R.grad_bias_bound(t["dy"].flatten(0, -2), dt)
        err = (gb.double().cpu() - total).abs()
        print(name, "grad_bias err / bound", float((err / bound).max()))
        assert gb.dtype == dt and (err <= bound).all(), (name, "grad_bias")


@pytest.mark.parametrize("name", NAMES)
def test_ckpt_variant_is_bit_identical_and_saves_codes_only(name):
    T = _train()
    meta, t, d = fixture(name)
    need = tuple(meta["need"])
    plain = run(T.int8_matmul_dynamic_with_backward, d, need)
    ckpt = run(T.int8_matmul_dynamic_with_backward_ckpt, d, need)
    for a, b in zip(plain, ckpt):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(bits(a), bits(b))
    x, w = d["x"].detach().clone().requires_grad_(need[0]), d["w"].detach().clone().requires_grad_(need[1])
    y = T.int8_matmul_dynamic_with_backward_ckpt(x, w, d.get("bias"))
    saved = [s for s in y.grad_fn.saved_tensors if s is not None]
    assert len(saved) == 2 * (need[0] + need[1])
    for s in saved:  # int8 codes and float32 scale vectors: no 16- or 32-bit copy of x or W
        assert s.dtype == torch.int8 or (s.dtype == torch.float32 and s.numel() == meta["K"]), (s.dtype, tuple(s.shape))
    assert sum(s.numel() for s in saved if s.dtype == torch.int8) <= (need[1] * (meta["M"] + 15) + need[0] * meta["N"]) * meta["K"]
    y = T.int8_matmul_dynamic_with_backward(x, w, d.get("bias"))
    assert {s.dtype for s in y.grad_fn.saved_tensors if s is not None} == {d["x"].dtype}


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (True, True, False), (False, False, True), (False, True, True)])
def test_needs_input_grad_subsets(need):
    T = _train()
    meta, t, d = fixture("bf16_m72_3d")
    for fn in (T.int8_matmul_dynamic_with_backward, T.int8_matmul_dynamic_with_backward_ckpt):
        full = run(fn, d, (True, True, True))
        part = run(fn, d, need)
        assert torch.equal(full[0], part[0])
        for n, f, p in zip(need, full[1:], part[1:]):
            assert (p is not None) == n
            if n:
                assert torch.equal(bits(f), bits(p))


def test_linear_forward_functions():
    """quantized_linear_forward_int8_matmul_dynamic[_ckpt] as a Linear's forward: the matmul from 32 rows on, F.linear below (the
    reference's rule), gradients on the module's parameters."""
    T = _train()
    meta, t, d = fixture("f16_m300_3d")
    lin = torch.nn.Linear(meta["K"], meta["N"]).to(DEV, torch.float16)
    with torch.no_grad():
        lin.weight.copy_(d["w"])
        lin.bias.copy_(d["bias"])
    for fwd, fn in ((T.quantized_linear_forward_int8_matmul_dynamic, T.int8_matmul_dynamic_with_backward),
                    (T.quantized_linear_forward_int8_matmul_dynamic_ckpt, T.int8_matmul_dynamic_with_backward_ckpt)):
        lin.zero_grad()
        y = fwd(lin, d["x"])
        assert torch.equal(y, fn(d["x"], lin.weight, lin.bias)) and torch.equal(y, T.int8_matmul_dynamic(d["x"], lin.weight, lin.bias))
        y.backward(d["dy"])
        assert lin.weight.grad.shape == lin.weight.shape and lin.bias.grad.shape == lin.bias.shape
        few = d["x"][0, :31]
        assert torch.equal(fwd(lin, few), torch.nn.functional.linear(few, lin.weight, lin.bias))
    with pytest.raises(NotImplementedError, match="N % 16"):
        T.int8_matmul_dynamic_with_backward(d["x"][..., :72], d["w"][:, :72], None)


def test_float32_master_weights_under_16_bit_activations():
    """Operands of different dtypes, as the reference accepts them (every operand is upcast to float32 before it is quantized): y and
    grad_input in the input's dtype, grad_weight and grad_bias computed in grad_output's dtype and handed to the float32 parameters.
    Each equals the same kernels called on the operands directly."""
    ops, T = _ops(), _train()
    meta, t, d = fixture("bf16_m72_3d")
    x2d, dy2d = d["x"].flatten(0, -2), d["dy"].flatten(0, -2)
    w32, b32 = d["w"].float() * 1.001, d["bias"].float() * 1.001  # values that bf16 does not hold
    xq, xs, _, _ = ops.rowquant(x2d, ops.MM_I8)
    wq, ws, _, _ = ops.rowquant(w32, ops.MM_I8)
    gq, gs, _, _ = ops.rowquant(dy2d, ops.MM_I8)
    wq_t, wsc, _ = ops.colquant_t(w32)
    xq_t, xsc, _ = ops.colquant_t(x2d)
    gq_t, gsc, colsum = ops.colquant_t(dy2d, want_colsum=True)
    want = (ops.scaled_mm(ops.MM_I8, xq, wq, xs, ws, b32, torch.bfloat16), ops.scaled_mm(ops.MM_I8, gq, wq_t, gs, wsc, None, torch.bfloat16),
            ops.scaled_mm(ops.MM_I8, gq_t, xq_t, gsc, xsc, None, torch.bfloat16).float(), colsum.to(torch.bfloat16).float())
    for fn in (T.int8_matmul_dynamic_with_backward, T.int8_matmul_dynamic_with_backward_ckpt):
        got = run(fn, {"x": d["x"], "w": w32, "bias": b32, "dy": d["dy"]}, (True, True, True))
        assert [g.dtype for g in got] == [torch.bfloat16, torch.bfloat16, torch.float32, torch.float32]
        for g, w in zip(got, want):
            assert torch.equal(g.reshape(w.shape), w)


@pytest.mark.parametrize("variant", ["plain", "ckpt"])
def test_captured_forward_backward_replays_to_the_eager_bits(variant):
    T = _train()
    fn = T.int8_matmul_dynamic_with_backward if variant == "plain" else T.int8_matmul_dynamic_with_backward_ckpt
    meta, t, d = fixture("bf16_m300")
    eager = run(fn, d, (True, True, True))
    x, w, b = (d[k].detach().clone().requires_grad_(True) for k in ("x", "w", "bias"))
    dy = d["dy"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture, as torch's graph recipe asks
        torch.autograd.grad(fn(x, w, b), (x, w, b), dy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fn(x, w, b)
        grads = torch.autograd.grad(y, (x, w, b), dy)
    with torch.no_grad():  # other values in the static buffers, then the fixture's again: the replay recomputes everything
        x.mul_(-1.5)
        dy.mul_(0.5)
        graph.replay()
        x.copy_(d["x"])
        dy.copy_(d["dy"])
        graph.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, (y,) + tuple(grads)):
        assert torch.equal(bits(a), bits(c.detach()))


def test_sgd_loop_tracks_float32_linear():
    """Ten SGD steps on a 64 -> 64 layer with 128 tokens: the MSE loss falls and stays within 2 % of the same loop on F.linear in float32
    (a sanity check at the level of the reference's own gradient error, 0.8-1.0 % rel-L2 per product, not a precision claim)."""
    T = _train()

    def loop(fn):
        g = torch.Generator().manual_seed(11)
        x = torch.randn(128, 64, generator=g).to(DEV)
        w = (torch.randn(64, 64, generator=g) * 0.1).to(DEV).requires_grad_(True)
        b = torch.zeros(64, device=DEV, requires_grad=True)
        target = (x @ (torch.randn(64, 64, generator=g) * 0.2).to(DEV) + 0.3).detach()
        losses = []
        for _ in range(10):
            loss = torch.nn.functional.mse_loss(fn(x, w, b), target)
            gw, gb = torch.autograd.grad(loss, (w, b))
            with torch.no_grad():
                w -= 8.0 * gw
                b -= 8.0 * gb
            losses.append(loss.item())
        return losses
    ref = loop(torch.nn.functional.linear)
    for fn in (T.int8_matmul_dynamic_with_backward, T.int8_matmul_dynamic_with_backward_ckpt):
        mine = loop(fn)
        print("losses", mine, ref)
        assert mine[-1] < 0.5 * mine[0]
        for a, r in zip(mine, ref):
            assert abs(a - r) <= 0.02 * r, (mine, ref)
