"""Int8 training Linear, host side: the CPU restatement (tests/train_linear_util.py) against the reference's fixtures
(tests/golden/train_int8_*), the argument checks of sdnq_hip_colquant_t, the import-name drop-in and what raises."""
import ctypes
import importlib
import types

import pytest
import torch

from tests import train_linear_util as R

QUANTS = {"fwd_x": ("x", -1), "gi_dy": ("dy", -1), "gi_w": ("w", 0), "gw_x": ("x", 0)}


@pytest.mark.parametrize("name", R.train_names())
def test_restatement_reproduces_codes_and_scales(name):
    meta, t = R.load(name)
    two_d = {"x": t["x"].flatten(0, -2), "dy": t["dy"].flatten(0, -2), "w": t["w"]}
    for key, (src, dim) in QUANTS.items():
        q, s = R.quantize(two_d[src], dim)
        assert torch.equal(q, t[key + "_q"]) and torch.equal(s, t[key + "_s"]), (name, key)
    q, s = R.quantize(t["w"], -1)                       # the forward's weight operand: the reference quantizes w.t() along dim 0
    assert torch.equal(q.t(), t["fwd_w_q"]) and torch.equal(s.t(), t["fwd_w_s"]), (name, "fwd_w")
    for src, key in (("dy", "gw_dy"), ("x", "gw_x"), ("w", "gi_w")):   # the transposed, zero-padded form of the column quantizer
        q_t, s, _ = R.colquant_t(two_d[src])
        r = two_d[src].shape[0]
        ref_q = t[key + "_q"] if key == "gw_dy" else t[key + "_q"].t()
        assert q_t.shape[1] % 16 == 0 and torch.equal(q_t[:, :r], ref_q) and not q_t[:, r:].any(), (name, key)
        assert torch.equal(s.reshape(-1), t[key + "_s"].reshape(-1)), (name, key)


@pytest.mark.parametrize("name", R.train_names())
def test_restatement_reproduces_outputs(name):
    meta, t = R.load(name)
    need = tuple(meta["need"])
    R.assert_w8a8_close(R.forward(t["x"], t["w"], t.get("bias")), t["y"], (name, "y"))
    gi, gw, gb = R.backward(t["x"], t["w"], t["dy"], need)
    for key, mine in (("grad_input", gi), ("grad_weight", gw)):
        assert (mine is None) == (key not in t), (name, key)
        if mine is not None:
            R.assert_w8a8_close(mine, t[key], (name, key))
    assert (gb is None) == ("grad_bias" not in t)
    if gb is not None:
        s, bound = R.grad_bias_bound(t["dy"].flatten(0, -2), gb.dtype)
        for mine in (gb, t["grad_bias"]):  # one rounding to the dtype on top of the float32 accumulation bound
            assert ((mine.double() - s).abs() <= bound).all(), (name, "grad_bias")


def test_fixtures_cover_the_issue_range():
    metas = [R.load(n)[0] for n in R.train_names()]
    assert {"bf16", "f16", "f32"} <= {m["dtype"] for m in metas}
    assert {33, 72} <= {m["M"] for m in metas}                                            # M % 16 != 0
    assert any(m["M"] > 2 * R.STAT_SLAB_ROWS and m["M"] > R.ROW_TILE for m in metas)      # several slabs of both kernels
    assert any(m["N"] % R.COLUMN_TILE and m["K"] % R.COLUMN_TILE for m in metas)          # a partial column tile
    assert any(len(m["tensors"]["x"]["shape"]) == 3 for m in metas)
    assert any("bias" not in m["tensors"] for m in metas)
    assert {(True, False, False), (False, True, False), (True, True, False)} <= {tuple(m["need"]) for m in metas}
    assert all(33 <= m["M"] <= 300 and 48 <= m["N"] <= 96 and 64 <= m["K"] <= 128 for m in metas)
    ties = [m for m in metas if m["name"] == "ties"][0]["ties"]
    assert min(ties.values()) > 1000
    assert all(sum(m["ties"].values()) >= 3 for m in metas if m["dtype"] == "bf16")      # bf16 data ties on its own
    assert all(m["ckpt_identical"] for m in metas)


def test_colquant_t_argument_validation_without_gpu():
    from sdnq_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    f, wsb = lib.sdnq_hip_colquant_t, lib.sdnq_hip_colquant_t_workspace_bytes
    ws = wsb(40, 64)
    assert ws > 0 and wsb(40, 60) == -3 and wsb(0, 64) == -3
    ok = dict(x=p, dt=1, r=40, c=64, ldx=64, xq=p, ld_t=48, xs=p, colsum=None, ws=p, wsb=ws, stream=None)

    def rc(**broken):
        return f(*{**ok, **broken}.values())
    assert rc(x=None) == -1 and rc(xq=None) == -1 and rc(xs=None) == -1 and rc(ws=None) == -1   # NULL
    assert rc(dt=7) == -2 and rc(dt=-1) == -2                                                     # dtype
    assert rc(c=60, ldx=60) == -3                                                                 # C % 8
    assert rc(ldx=56) == -3                                                                       # ldx < C
    assert rc(ld_t=32) == -3                                                                      # ld_t < R
    assert rc(ld_t=40) == -3                                                                      # ld_t % 16
    assert rc(x=p + 2) == -4 and rc(xq=p + 8) == -4 and rc(ws=p + 4) == -4                        # misaligned pointers
    assert rc(ldx=68) == -4                                                                       # bf16 rows of 136 bytes
    assert rc(wsb=ws - 1) == -3 and rc(wsb=0) == -3                                               # short workspace
    assert wsb(16384, 3072) < 16384 * 3072 // 8                                                   # partials, not a copy


ALL_CQ_SHAPES = {**R.CENSUS_SHAPES, **R.EDGE_SHAPES}


@pytest.mark.parametrize("shape", list(ALL_CQ_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_cq_plan_restatement_and_the_regimes_of_the_training_size_shapes(shape):
    """tests/test_colquant_exact_gpu.py picks its shapes by the regime of csrc/colquant.hip they reach.  The restated plan gives the
    library's workspace size (2 partials per slab and column), and every shape reaches what the table in train_linear_util says."""
    from sdnq_amd import _lib
    r, c = shape
    ctiles, nslab, slab_rows = R.cq_plan(r, c)
    assert 2 * nslab * c * 4 == _lib.load().sdnq_hip_colquant_t_workspace_bytes(r, c)
    assert slab_rows % R.STAT_SLAB_ROWS == 0 and (nslab - 1) * slab_rows < r <= nslab * slab_rows and nslab <= R.MAX_SLABS
    assert R.regime(r, c) == ALL_CQ_SHAPES[shape]


def test_training_size_shapes_cover_what_the_fixtures_leave_out():
    got = [R.regime(*s) for s in ALL_CQ_SHAPES]
    assert {1, 2, 3} <= {g["passes"] for g in got}                       # the statistics loop runs once, twice, three times per slab
    assert max(g["nslab"] for g in got) == R.MAX_SLABS                   # the slab reduction at its maximum ...
    assert {1, 16} <= {g["want"] for g in got}                           # ... and cut short by many column tiles (want < 32)
    assert sum(g["last_slab"] == 1 for g in got) >= 2                    # a last slab of one row
    assert max(g["row_tiles"] for g in got) >= 33 and any(s[0] % 256 == 1 for s in ALL_CQ_SHAPES)   # a last row tile of one row
    assert any(s[1] == 8 for s in ALL_CQ_SHAPES) and max(g["ctiles"] for g in got) == 512
    for name in R.train_names():                                         # what the fixtures reach: one pass, three slabs, two row tiles
        meta = R.load(name)[0]
        for c in (meta["N"], meta["K"]):
            g = R.regime(meta["M"], c)
            assert g["passes"] == 1 and g["nslab"] <= 3 and g["row_tiles"] <= 2 and g["want"] == 32


@pytest.mark.parametrize("shape", list(R.CENSUS_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_matrix_is_exact_and_the_oracle_returns_its_codes(shape):
    """The constructed census input: a value of all three dtypes, every entry non-zero, one +-127 per column at the pinned row -- one in
    each third of the columns at row 0, at row R - 1 and in a later pass of a slab -- and the C oracle gives back q and 2^e."""
    r, c = shape
    pins = R.census_pin_rows(r, c)
    x, q, e = R.exact_matrix(r, c, torch.Generator().manual_seed(r + c), None, pins)
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(x.to(dt).float(), x)
    assert q.dtype == torch.int8 and (q != 0).all() and torch.equal(x.double(), q.double() * torch.exp2(e.double()))
    big = q.abs() == 127
    assert (big.sum(0) == 1).all() and big[pins, torch.arange(c)].all() and (q.abs()[~big] <= 8).all()
    assert e.min() >= -3 and e.max() <= 3 and len(set(e.tolist())) > 1
    _, nslab, slab_rows = R.cq_plan(r, c)
    cycle = 3 if slab_rows >= 256 else 2
    assert (pins[0::cycle] == 0).all() and (pins[1::cycle] == r - 1).all() and (r - 1) // slab_rows == nslab - 1
    if cycle == 3:
        later = pins[2::3]
        assert ((later % slab_rows >= 128) & (later < r)).all() and len(set((later // slab_rows).tolist())) >= min(nslab, len(later), 4)
    assert (x.double().sum(0).abs() < 2.0 ** 24 * torch.exp2(e.double())).all() and torch.equal(x.sum(0).double(), x.double().sum(0))
    codes, scale = R.oracle_colquant_t(x)
    assert torch.equal(codes[:, :r], q.t()) and not codes[:, r:].any() and torch.equal(scale.reshape(-1), torch.exp2(e.float()))


def test_oracle_column_quantizer_agrees_with_the_restatement_on_the_edge_matrices():
    """Two independent CPU implementations, bit for bit, on the inputs the GPU tests hold the kernel to the oracle on."""
    from tests import rowquant_inputs
    wide = torch.from_numpy(rowquant_inputs.exponent_range()).t()
    for x in (torch.from_numpy(rowquant_inputs.ties_and_near_ties()).t(), wide, wide.to(torch.bfloat16)):
        codes, scale = R.oracle_colquant_t(x)
        q_t, s, _ = R.colquant_t(x.contiguous())
        assert torch.equal(codes, q_t) and torch.equal(scale.view(torch.int32), s.view(torch.int32))


def test_oracle_chain_agrees_with_the_restatement_on_exact_operands():
    """The chain of the exact-sum GPU test at a small size: the oracle's three products equal the float64 products rounded once."""
    g = torch.Generator().manual_seed(5)
    (x, _), (w, _), (dy, _) = R.exact_operand(72, 48, g, -2), R.exact_operand(32, 48, g, -5), R.exact_operand(72, 32, g, -1)
    bias = torch.randint(-64, 65, (32,), generator=g).float() * 2.0 ** -7
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        y, gi, gw = R.oracle_chain(x.to(dt), w.to(dt), bias.to(dt), dy.to(dt), dt)
        want = ((x.double() @ w.double().t() + bias.double()), dy.double() @ w.double(), dy.double().t() @ x.double())
        for got, ref in zip((y, gi, gw), want):
            assert torch.isfinite(ref.to(dt)).all() and torch.equal(got, ref.to(dt))


def test_import_name_drop_in():
    import importlib

    from sdnq_amd import training as T
    dyn = importlib.import_module("sdnq.training.layers.linear.linear_int8.linear_int8_dynamic")
    ckpt = importlib.import_module("sdnq.training.layers.linear.linear_int8.linear_int8_dynamic_ckpt")
    assert dyn.int8_matmul_dynamic_with_backward is T.int8_matmul_dynamic_with_backward
    assert dyn.int8_matmul_dynamic is T.int8_matmul_dynamic
    assert dyn.quantized_linear_forward_int8_matmul_dynamic is T.quantized_linear_forward_int8_matmul_dynamic
    assert ckpt.int8_matmul_dynamic_with_backward_ckpt is T.int8_matmul_dynamic_with_backward_ckpt
    assert ckpt.quantized_linear_forward_int8_matmul_dynamic_ckpt is T.quantized_linear_forward_int8_matmul_dynamic_ckpt
    assert dyn.INT8MatmulDynamicBackward is T.INT8MatmulDynamicBackward and ckpt.INT8MatmulDynamicBackwardCKPT is T.INT8MatmulDynamicBackwardCKPT


def test_cpu_tensors_and_unbuilt_configurations_raise():
    from sdnq_amd import _lib, training as T
    x, w, b = torch.randn(40, 64), torch.randn(48, 64), torch.randn(48)
    for fn in (T.int8_matmul_dynamic_with_backward, T.int8_matmul_dynamic_with_backward_ckpt, T.int8_matmul_dynamic):
        with pytest.raises(_lib.SdnqHipError, match="CPU"):
            fn(x, w, b)
    layer = types.SimpleNamespace(weight=w, bias=b)
    for fwd in (T.quantized_linear_forward_int8_matmul_dynamic, T.quantized_linear_forward_int8_matmul_dynamic_ckpt):
        with pytest.raises(_lib.SdnqHipError, match="CPU"):
            fwd(layer, x)
        assert torch.equal(fwd(layer, x[:8]), torch.nn.functional.linear(x[:8], w, b))   # fewer than 32 rows: the reference's own rule

    class SDNQTensor:  # stands for the reference's quantized weight subclass
        sdnq_dequantizer = object()
        shape, ndim, dtype, is_cuda = (48, 64), 2, torch.float32, True
    with pytest.raises(NotImplementedError, match="SDNQTensor"):
        T.int8_matmul_dynamic_with_backward(x, SDNQTensor(), None)
    with pytest.raises(NotImplementedError, match="SDNQTensor"):
        T.quantized_linear_forward_int8_matmul_dynamic(types.SimpleNamespace(weight=SDNQTensor(), bias=None), x[:8])
    with pytest.raises(NotImplementedError, match="use_sr"):
        T.int8_matmul_dynamic(x, w, b, use_sr=True)
    with pytest.raises(NotImplementedError, match="SVD"):
        T.int8_matmul_dynamic(x, w, b, svd_up=w, svd_down=w)
    with pytest.raises(NotImplementedError, match="Hadamard"):
        T.int8_matmul_dynamic(x, w, b, hadamard=w)
    # the shape and dtype rules come after the device check: stand-ins that say they are on the device
    with pytest.raises(NotImplementedError, match="N % 16"):
        T._check(types.SimpleNamespace(dtype=torch.float32, is_cuda=True, shape=(40, 64)),
                 types.SimpleNamespace(dtype=torch.float32, is_cuda=True, shape=(40, 64), ndim=2), None)
    with pytest.raises(NotImplementedError, match="N % 16"):
        T._check(types.SimpleNamespace(dtype=torch.float32, is_cuda=True, shape=(40, 72)),
                 types.SimpleNamespace(dtype=torch.float32, is_cuda=True, shape=(48, 72), ndim=2), None)
    with pytest.raises(NotImplementedError, match="float32 / bfloat16 / float16"):
        T._check(types.SimpleNamespace(dtype=torch.float64, is_cuda=True, shape=(40, 64)),
                 types.SimpleNamespace(dtype=torch.float64, is_cuda=True, shape=(48, 64), ndim=2), None)
    # the reference's other training matmuls answer by name at the reference's own module paths
    assert len(T.NOT_BUILT) == 14
    for name in T.NOT_BUILT:
        family = "linear_" + name.split("_")[0]
        module = family + ("_dynamic" if "_dynamic_" in name else "") + ("_ckpt" if name.endswith("_ckpt") else "")
        fn = getattr(importlib.import_module(f"sdnq.training.layers.linear.{family}.{module}"), name)
        assert fn is getattr(T, name)
        with pytest.raises(NotImplementedError, match=name):
            fn(x, w, b)
