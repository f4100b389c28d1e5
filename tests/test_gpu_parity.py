"""GPU parity tests (run on the MI355X box with ``-m gpu``): the HIP path, called through the C ABI, against
(1) the golden vectors captured from the reference and (2) the CPU oracle on seeded inputs.

Tolerances (written here):
  * unpack / dequant (fp32 path) / re-quant / activation quantization / int8 matmul: BIT-EXACT;
  * asymmetric dequant: fma == CPU addcmul -> bit-exact as well;
  * SVD dequant (addmm in bf16): <= 1 bf16 ulp;
  * Hadamard in bf16/f16: <= 1 ulp of the dtype on rare elements (summation order), f32: ~1e-6 relative;
  * fp8 matmul / bf16 float GEMM: fp32 accumulation-order noise, then ONE rounding to the output dtype:
    |err| <= 2 ulp(out dtype) of the output's magnitude scale, rel-L2 <= 2e-3 (bf16) / 1e-5 (f32).
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import rowquant_inputs
from tests.golden_util import GOLD, Case, case_names
from tests.modules_util import TORCH_DT, module_from_case, to_f32_numpy

pytestmark = pytest.mark.gpu

from sdnq_amd import ops  # noqa: E402


def bits_of(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy()
    if t.dtype in (torch.float8_e4m3fn, torch.int8):
        return t.view(torch.uint8).numpy()
    return t.numpy()


def assert_close_float(got: np.ndarray, ref: np.ndarray, tag: str, what, hadamard=False, f32_lim=2e-6, f16mm=False):
    """f16mm: the float16 matmul forward.  The reference's CPU route (the fixtures, the oracle) rounds BOTH operands to float16 a second
    time after its 1 / sqrt(65536 K) pre-scaling and rounds the accumulated dot product to float16 (kernel_wrappers.py:115-129); the
    matrix cores accumulate the once-rounded operands in float32 (what the reference's Triton route does): three 2^-11 roundings apart."""
    scale = float(np.abs(ref).max()) or 1.0
    err = float(np.abs(got - ref).max()) / scale
    lim = {"bf16": 2 * 2.0 ** -8, "f16": (8 if f16mm else 2) * 2.0 ** -11, "f32": f32_lim}[tag] * (2.0 if hadamard else 1.0)
    assert err <= lim, (what, "max err / scale", err, lim)
    l2 = float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) or 1.0))
    assert l2 <= {"bf16": 2e-3, "f16": (2e-3 if f16mm else 5e-4), "f32": max(1e-5, f32_lim)}[tag], (what, "rel l2", l2)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_module_forward_vs_golden_and_oracle(name, gpu_device):
    c = Case(name)
    d = c.deq
    mod = module_from_case(c, gpu_device)
    omod = c.oracle_module()
    for M in c.ms():
        x = c.torch_tensor(f"x_{M}", device=gpu_device)
        y = mod(x)
        assert y.dtype == x.dtype and tuple(y.shape) == tuple(c.info(f"y_{M}")["shape"])
        got = to_f32_numpy(y)
        ref = c.f32(f"y_{M}")
        orc = O.forward(omod, c.f32(f"x_{M}"), c.tag)
        qmm = d["use_quantized_matmul"] and M >= 32
        exact = qmm and d["quantized_matmul_dtype"] in ("int8", "uint8") and not d["use_hadamard"] and not c.has("svd_up")
        if exact:
            assert np.array_equal(got, ref), (name, M, "vs golden", int((got != ref).sum()))
            assert np.array_equal(got, orc), (name, M, "vs oracle")
        else:
            f16mm = qmm and d["quantized_matmul_dtype"] == "float16"
            assert_close_float(got, ref, c.tag, (name, M, "golden"), hadamard=d["use_hadamard"], f16mm=f16mm)
            assert_close_float(got, orc, c.tag, (name, M, "oracle"), hadamard=d["use_hadamard"], f16mm=f16mm)


@pytest.mark.parametrize("name", ["fp8_f16mm_bf16", "float6_e3m2_f16mm_f16_nobias", "int8_f16mm_bf16", "uint4_group32_f16mm_hadamard_f16", "int8_svd_f16mm_bf16"])
def test_float16_matmul_operators_vs_oracle(name, gpu_device):
    """The three pieces of the float16 matmul forward (round 6; linear_fp16.py): the activation quantizer and the weight operand are
    elementwise and must equal the oracle (= the reference's) bit for bit; the scaled matmul is checked against a float64 evaluation of
    fma(acc * sa, sb, bias) on the SAME float16 operands: float32 accumulation error only (2 sqrt(K) 2^-24 of the row's magnitude)."""
    from sdnq_amd import linear as L, ops
    c = Case(name)
    mod = module_from_case(c, gpu_device)
    omod = c.oracle_module()
    d = c.deq
    mod(c.torch_tensor(f"x_{max(c.ms())}", device=gpu_device))  # builds the cached weight operand: stored codes, or re-quantized to float16 codes
    st = L._state(mod)
    w16, wsc = st.mm_weight, st.mm_scale
    for M in [m for m in c.ms() if m >= 32]:
        x = c.torch_tensor(f"x_{M}", device=gpu_device)
        x2 = x.reshape(-1, c.K)
        _, inter = O.forward(omod, c.f32(f"x_{M}"), c.tag, want_intermediates=True)
        assert np.array_equal(w16.cpu().numpy().view(np.uint16), inter["wq"].view(np.uint16)), (name, "weight operand")
        assert np.array_equal(wsc.cpu().numpy().reshape(-1), np.asarray(inter["ws"], dtype=np.float32).reshape(-1)), (name, "weight scales")
        if d["use_hadamard"] or c.has("svd_up"):
            continue  # (the rotated input differs by the dtype's rounding of another summation order: covered by the forward test)
        xq, xs = ops.rowquant_f16(x2)
        assert np.array_equal(xq.cpu().numpy().view(np.uint16), inter["xq"].view(np.uint16)), (name, M, "float16 codes")
        assert np.array_equal(xs.cpu().numpy(), inter["xs"]), (name, M, "row scales")
        for out_dtype, tag in ((torch.float32, "f32"), (x.dtype, c.tag)):
            y = ops.scaled_mm_f16(xq, w16, xs, wsc, mod.bias, out_dtype)
            acc = inter["xq"].astype(np.float64) @ inter["wq"].astype(np.float64).T
            want = acc * inter["xs"].astype(np.float64)[:, None] * inter["ws"].astype(np.float64).reshape(1, -1)
            if mod.bias is not None:
                want = want + mod.bias.detach().float().cpu().numpy().astype(np.float64).reshape(1, -1)
            got = to_f32_numpy(y).astype(np.float64)
            mag = (np.abs(inter["xq"].astype(np.float64)) @ np.abs(inter["wq"].astype(np.float64)).T) * inter["xs"].astype(np.float64)[:, None] \
                * np.abs(inter["ws"].astype(np.float64)).reshape(1, -1) + 1e-30
            lim = 2 * np.sqrt(c.K) * 2.0 ** -24 * mag + {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[tag] * np.abs(want) + 1e-30
            assert np.all(np.abs(got - want) <= lim), (name, M, tag, float((np.abs(got - want) / lim).max()))
    # a NaN / all-zero row: nan_to_num and the clamp
    xz = torch.zeros(40, c.K, device=gpu_device, dtype=torch.bfloat16)
    xz[3, 5] = float("nan")
    xz[7, :] = 3.0
    q, s = ops.rowquant_f16(xz)
    assert torch.all(q[0] == 0) and s[0].item() == 0.0 and torch.isnan(s[3]) and torch.all(q[3] == 0) and torch.all(q[7] == 65504.0)


@pytest.mark.parametrize("m,n,k", [(4096, 2560, 1024), (4096, 5120, 320), (300, 264, 200), (64, 128, 4104)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_float16_scaled_mm_all_tiles(m, n, k, out_dtype, gpu_device):
    """Every tile shape of sdnq_hip_scaled_mm_f16 (256x256 half-tile ring, 256x128, 64x128, 64x64; ragged M / N / K) against float64 on the
    same operands: float32 accumulation error (2 sqrt(K) 2^-24 of sum|a||b|) plus the output rounding."""
    from sdnq_amd import ops
    g = torch.Generator(device="cpu").manual_seed(m + n + k)
    a = (torch.randn(m, k, generator=g) * 3000).to(torch.float16).to(gpu_device)
    b = (torch.randn(n, k, generator=g) * 20).to(torch.float16).to(gpu_device)
    sa = (torch.rand(m, generator=g) * 1e-4 + 1e-5).to(gpu_device)
    sb = (torch.rand(n, generator=g) * 1e-2 + 1e-3).to(gpu_device)
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(gpu_device)
    for bs in (bias, None):
        y = ops.scaled_mm_f16(a, b, sa, sb, bs, out_dtype).double()
        want = (a.double() @ b.double().t()) * sa.double()[:, None] * sb.double()[None, :]
        mag = (a.double().abs() @ b.double().abs().t()) * sa.double()[:, None] * sb.double()[None, :]
        if bs is not None:
            want = want + bs.double()[None, :]
        lim = 2 * (k ** 0.5) * 2.0 ** -24 * mag + (2.0 ** -8 if out_dtype == torch.bfloat16 else 2.0 ** -23) * want.abs() + 1e-30
        assert bool(((y - want).abs() <= lim).all()), (m, n, k, out_dtype, float(((y - want).abs() / lim).max()))


@pytest.mark.parametrize("name", ["int8_rowwise_qmm_bf16", "int8_rowwise_qmm_f16_nobias", "uint4_qmm_bf16", "int8_svd32_qmm_bf16",
                                  "int8_rowwise_noqmm_bf16", "fp8_qmm_bf16", "int6_rowwise_packed_qmm_bf16",
                                  "uint8_uint8mm_qmm_bf16", "uint4_uint8mm_qmm_bf16", "int8_group64_uint8mm_qmm_bf16", "uint8_uint8mm_qmm_bf16_k384"])
def test_apply_options_dequantize_fp32_false(name, gpu_device):
    """A float32-scale checkpoint switched to model-dtype scales by apply_sdnq_options_to_model(dequantize_fp32=False) (loader.py:
    262-283) computes what the oracle's 16-bit-scale restatement (pinned by the *_lpscale fixtures) gives for the re-typed layer."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    c = Case(name)
    mod = module_from_case(c, gpu_device)
    model = torch.nn.Sequential(mod)
    sdnq_amd.apply_sdnq_options_to_model(model, dequantize_fp32=False)
    assert mod.scale.dtype == mod.sdnq_dequantizer.result_dtype != torch.float32
    omod = oracle_from_module(mod)
    assert omod.scale_tag == c.tag
    d = c.deq
    for M in c.ms():
        x = c.torch_tensor(f"x_{M}", device=gpu_device)
        got = to_f32_numpy(model(x))
        orc = O.forward(omod, c.f32(f"x_{M}"), c.tag)
        qmm = d["use_quantized_matmul"] and M >= 32
        if qmm and d["quantized_matmul_dtype"] in ("int8", "uint8") and not c.has("svd_up"):
            assert np.array_equal(got, orc), (name, M, int((got != orc).sum()))
        else:
            assert_close_float(got, orc, c.tag, (name, M, "oracle"))
    sdnq_amd.apply_sdnq_options_to_model(model, dequantize_fp32=True)  # and back: float32 scales (values stay the rounded ones)
    assert mod.scale.dtype == torch.float32
    assert model(c.torch_tensor(f"x_{c.ms()[-1]}", device=gpu_device)).dtype == mod.sdnq_dequantizer.result_dtype


@pytest.mark.parametrize("name", case_names())
def test_dequant_and_requant_vs_golden(name, gpu_device):
    c = Case(name)
    mod = module_from_case(c, gpu_device)
    dq = mod.sdnq_dequantizer
    # fp32, Hadamard not undone: the tensor re_quantize_matmul starts from
    w32 = dq(mod.weight, mod.scale, zero_point=mod.zero_point, svd_up=mod.svd_up, svd_down=mod.svd_down,
             skip_quantized_matmul=dq.use_quantized_matmul, dtype=torch.float32, non_hadamard=True)
    ref32 = c.f32("w_dequant_f32_nohad").reshape(c.N, c.K)
    got32 = to_f32_numpy(w32).reshape(c.N, c.K)
    if c.has("svd_up"):
        # addmm in the svd dtype: <= 1 ulp(16-bit) of the RESULT; results that cancel to ~0 get the absolute floor the oracle's own
        # golden test uses (the ulp of a cancelled result says nothing about the rounding of its addends)
        assert np.all(np.abs(got32 - ref32) <= np.maximum(np.abs(ref32) * 2.0 ** -7, 1e-8)), name
        assert np.mean(got32 != ref32) < 1e-3, name
    else:
        assert np.array_equal(got32, ref32), (name, int((got32 != ref32).sum()))
    # result dtype, as SDNQLayer.dequantize() produces it
    w = dq(mod.weight, mod.scale, zero_point=mod.zero_point, svd_up=mod.svd_up, svd_down=mod.svd_down,
           skip_quantized_matmul=dq.use_quantized_matmul)
    ref = c.f32("w_dequant").reshape(c.N, c.K)
    got = to_f32_numpy(w).reshape(c.N, c.K)
    if dq.use_hadamard or c.has("svd_up"):
        assert np.all(np.abs(got - ref) <= 2 * np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7 + 1e-6), name
    else:
        assert np.array_equal(got, ref), name
    if c.has("requant_weight"):
        wq, ws, *wzp = dq.re_quantize_matmul(mod.weight, mod.scale, zero_point=mod.zero_point)
        assert tuple(wq.shape) == (c.K, c.N) and wq.stride() == (1, c.K)
        rw = c.raw("requant_weight").reshape(c.K, c.N)
        assert np.array_equal(bits_of(wq.contiguous()).view(np.uint8), rw.view(np.uint8)), name  # (int8 / e4m3 bytes, or float16 bit patterns)
        assert np.array_equal(ws.float().cpu().numpy().reshape(-1), c.f32("requant_scale").reshape(-1)), name
        assert len(wzp) == int(c.has("requant_zero_point")), name
        if wzp:  # asymmetric re-quantizer of the uint8 matmul (dequantizer.py:178-187)
            assert tuple(wzp[0].shape) == (1, c.N)
            assert np.array_equal(wzp[0].float().cpu().numpy().reshape(-1), c.f32("requant_zero_point").reshape(-1)), name  # (values: bf16 bits under 16-bit scales)


def test_dequant_every_storage_dtype_bit_exact(gpu_device):
    z = np.load(os.path.join(GOLD, "dequant_dtypes.npz"))
    meta = json.load(open(os.path.join(GOLD, "dequant_dtypes.json")))["dtypes"]
    from tests.modules_util import dequantizer_from_fields
    n_checked = 0
    for key, ent in meta.items():
        dq = dequantizer_from_fields(ent["deq"])
        wt = torch.from_numpy(z[f"{key}.weight"])
        tag = ent["tensors"]["weight"]["dtype"]
        view = {"fp8e4m3": torch.float8_e4m3fn, "fp8e5m2": torch.float8_e5m2, "f16": torch.float16, "bf16": torch.bfloat16}.get(tag)
        if view is not None:
            wt = wt.view(view)
        sc = torch.from_numpy(z[f"{key}.scale"]).to(gpu_device)
        zp = torch.from_numpy(z[f"{key}.zero_point"]).to(gpu_device) if ent["tensors"]["zero_point"]["dtype"] != "none" else None
        out = dq(wt.to(gpu_device), sc, zero_point=zp, dtype=torch.float32)
        ref = z[f"{key}.out"].reshape(16, 128)
        assert np.array_equal(out.cpu().numpy().reshape(16, 128), ref), key
        n_checked += 1
    assert n_checked >= 80


# ------------------------------------------------------------------------------------------------
_MM_I8_SHAPES = [(48, 256, 512), (77, 640, 2048), (333, 80, 48), (1000, 336, 144), (4096, 640, 640),
                 (129, 1280, 1280), (64, 64, 64), (32, 32, 32), (257, 2576, 656)]


# large shapes (M > 400) once, in bf16: the parameter list says so, nothing is skipped at run time
@pytest.mark.parametrize("shape,out_dt", [(sh, dt) for dt in (torch.bfloat16, torch.float16, torch.float32) for sh in _MM_I8_SHAPES
                                          if dt == torch.bfloat16 or sh[0] <= 400])
def test_scaled_mm_int8_bit_exact_vs_oracle(shape, out_dt, gpu_device):
    m, n, k = shape
    g = torch.Generator().manual_seed(m * 7 + n)
    a = torch.randint(-128, 128, (m, k), dtype=torch.int8, generator=g)
    b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g)
    sa = torch.rand(m, generator=g) * 0.02 + 1e-4
    sb = torch.rand(n, generator=g) * 0.02 + 1e-4
    tag = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[out_dt]
    for bias_mode in ("none", "1d", "2d"):
        bias = None if bias_mode == "none" else (torch.randn(n, generator=g) if bias_mode == "1d" else torch.randn(m, n, generator=g))
        bias_t = None if bias is None else bias.to(out_dt if bias_mode == "1d" else torch.float32)
        out = ops.scaled_mm(ops.MM_I8, a.to(gpu_device), b.to(gpu_device), sa.to(gpu_device), sb.to(gpu_device),
                            None if bias_t is None else bias_t.to(gpu_device), out_dt)
        ref = O.scaled_mm("int8", a.numpy(), b.numpy(), sa.numpy(), sb.numpy(),
                          None if bias_t is None else bias_t.float().numpy(), tag)
        got = to_f32_numpy(out)
        assert np.array_equal(got, ref), (shape, out_dt, bias_mode, int((got != ref).sum()))


@pytest.mark.parametrize("shape", [(48, 256, 512), (100, 64, 192), (256, 128, 1280), (77, 1280, 2048), (513, 336, 208)])
def test_scaled_mm_fp8_vs_oracle(shape, gpu_device):
    m, n, k = shape
    g = torch.Generator().manual_seed(11 + m)
    a = (torch.randn(m, k, generator=g) * 60).clamp(-448, 448).to(torch.float8_e4m3fn)
    b = (torch.randn(n, k, generator=g) * 60).clamp(-448, 448).to(torch.float8_e4m3fn)
    sa = torch.rand(m, generator=g) * 0.02 + 1e-4
    sb = torch.rand(n, generator=g) * 0.02 + 1e-4
    bias = torch.randn(n, generator=g).to(torch.bfloat16)
    for out_dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        out = ops.scaled_mm(ops.MM_FP8, a.to(gpu_device), b.to(gpu_device), sa.to(gpu_device), sb.to(gpu_device),
                            bias.to(gpu_device), out_dt)
        ref = O.scaled_mm("fp8", a.view(torch.uint8).numpy(), b.view(torch.uint8).numpy(), sa.numpy(), sb.numpy(),
                          bias.float().numpy(), tag)
        # fp32 output exposes the accumulator: the K=64 block-scaled fp8 MFMA sums its 64 products at reduced internal
        # width before the fp32 accumulate, so allow 1e-4 of the output scale there (bf16 output: 2 ulp as usual)
        assert_close_float(to_f32_numpy(out), ref, tag, (shape, tag), f32_lim=1e-4)


# the two large shapes once, in bf16
@pytest.mark.parametrize("m,k,dt", [(m, k, dt) for dt in (torch.bfloat16, torch.float16, torch.float32)
                                    for m, k in [(100, 640), (33, 1280), (7, 5120), (64, 48), (40, 15360), (4096, 640)]
                                    if dt == torch.bfloat16 or m * k <= 300000])
def test_rowquant_bit_exact_vs_oracle(m, k, dt, gpu_device):
    g = torch.Generator().manual_seed(k + m)
    x = torch.randn(m, k, generator=g) * 3
    x[:, 5 % k] *= 20
    x[min(3, m - 1)] = 0  # all-zero row: scale 0 -> q 0
    x = x.to(dt)
    xf = x.float().numpy()
    for mm, name in ((ops.MM_I8, "int8"), (ops.MM_FP8, "fp8")):
        xq, xs, rs, _ = ops.rowquant(x.to(gpu_device), mm, want_rowsum=(mm == ops.MM_I8))
        q, s, rowsum = O.rowquant(xf, name)
        assert np.array_equal(bits_of(xq), q.view(np.uint8)), (m, k, dt, name)
        assert np.array_equal(xs.cpu().numpy().reshape(-1), s), (m, k, dt, name)
        if rowsum is not None:
            assert np.array_equal(rs.cpu().numpy(), rowsum)


def test_rowquant_rounding_ties_and_near_ties(gpu_device):
    """Rows built so that MANY quotients x / scale are exact rounding ties (k + 0.5 -> half to even) or sit one ulp beside one:
    the codes must be the reference's bit for bit (any shortcut around the IEEE division would show here first)."""
    x = torch.from_numpy(rowquant_inputs.ties_and_near_ties())
    for asym in (False, True):
        if asym:
            got = ops.rowquant(x.to(gpu_device), ops.MM_I8, asymmetric=True)
            q, s_, zp = O.rowquant_asym(x.numpy())
            assert np.array_equal(got[4].cpu().numpy(), zp)
        else:
            got = ops.rowquant(x.to(gpu_device), ops.MM_I8, want_rowsum=True)
            q, s_, rowsum = O.rowquant(x.numpy(), "int8")
            assert np.array_equal(got[2].cpu().numpy(), rowsum)
        assert np.array_equal(bits_of(got[0]), q.view(np.uint8)), asym
        assert np.array_equal(got[1].cpu().numpy().reshape(-1), s_)


def test_asymmetric_rowquant_long_rows(gpu_device):
    """uint8-matmul activations (quantize_uint_mm_input) at FLUX row lengths: K = 12288 and 15360 (ff.out / proj_out) used to be
    refused beyond 5120 elements; the LDS-resident kernel has no such limit."""
    for k in (12288, 15360, 5128):
        g = torch.Generator().manual_seed(k)
        x = (torch.randn(33, k, generator=g) * 2 + 0.3).to(torch.bfloat16)
        xq, xs, rs, _, xzp = ops.rowquant(x.to(gpu_device), ops.MM_I8, want_rowsum=True, asymmetric=True)
        q, s_, zp = O.rowquant_asym(x.float().numpy())
        assert np.array_equal(bits_of(xq), q.view(np.uint8)) and np.array_equal(xs.cpu().numpy().reshape(-1), s_)
        assert np.array_equal(xzp.cpu().numpy(), zp) and np.array_equal(rs.cpu().numpy(), q.astype(np.int32).sum(-1))


@pytest.mark.parametrize("g_size", [4, 8, 16, 32, 64, 128, 256, 512])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_hadamard_vs_oracle(g_size, dt, gpu_device):
    tag = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[dt]
    k = g_size * 3 if g_size >= 8 else 24
    gen = torch.Generator().manual_seed(g_size)
    x = (torch.randn(37, k, generator=gen) * 2).to(dt)
    y = ops.hadamard(x.to(gpu_device), g_size)
    ref = O.rotate_hadamard(x.float().numpy(), g_size, tag)
    got = to_f32_numpy(y)
    ulp = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -21}[tag]
    assert np.all(np.abs(got - ref) <= 2 * ulp * np.maximum(np.abs(ref), np.abs(ref).max() * (1.0 if tag == "f32" else 0.0) + 1e-3)), (g_size, tag)
    if tag != "f32":
        assert np.mean(got != ref) < 0.02, (g_size, tag, float(np.mean(got != ref)))
    # involution: H is symmetric orthonormal, rotating twice returns the input (to rounding)
    if g_size in (4, 16, 64, 256) and tag == "f32":
        back = to_f32_numpy(ops.hadamard(y, g_size))
        assert np.allclose(back, x.float().numpy(), rtol=0, atol=1e-4)


# ------------------------------------------------------------------------------------------------
# size-independent properties at BASELINE sizes
# ------------------------------------------------------------------------------------------------
def test_int8_matmul_properties_at_sdxl_size(gpu_device):
    m, n, k = 4096, 5120, 640
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-128, 128, (m, k), dtype=torch.int8, generator=g).to(gpu_device)
    b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g).to(gpu_device)
    sa = (torch.rand(m, generator=g) * 0.02 + 1e-4).to(gpu_device)
    sb = (torch.rand(n, generator=g) * 0.02 + 1e-4).to(gpu_device)
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(gpu_device)
    full = ops.scaled_mm(ops.MM_I8, a, b, sa, sb, bias, torch.bfloat16)
    # (1) K-permutation invariance: int32 accumulation is exact
    perm = torch.randperm(k, generator=g).to(gpu_device)
    p = ops.scaled_mm(ops.MM_I8, a[:, perm].contiguous(), b[:, perm].contiguous(), sa, sb, bias, torch.bfloat16)
    assert torch.equal(full, p)
    # (2) row/column slices of the big problem equal the small problems (tile independence)
    rows = ops.scaled_mm(ops.MM_I8, a[1000:1077].contiguous(), b, sa[1000:1077].contiguous(), sb, bias, torch.bfloat16)
    assert torch.equal(full[1000:1077], rows)
    cols = ops.scaled_mm(ops.MM_I8, a, b[640:1280].contiguous(), sa, sb[640:1280].contiguous(), bias[640:1280].contiguous(), torch.bfloat16)
    assert torch.equal(full[:, 640:1280], cols)
    # (3) a sampled block against the oracle
    ref = O.scaled_mm("int8", a[:64].cpu().numpy(), b[:256].cpu().numpy(), sa[:64].cpu().numpy(), sb[:256].cpu().numpy(),
                      bias[:256].float().cpu().numpy(), "bf16")
    assert np.array_equal(to_f32_numpy(full[:64, :256]), ref)
    # (4) power-of-two scaling of sa is exact
    dbl = ops.scaled_mm(ops.MM_I8, a, b, sa * 2, sb, None, torch.float32)
    base = ops.scaled_mm(ops.MM_I8, a, b, sa, sb, None, torch.float32)
    assert torch.equal(dbl, base * 2)


def test_cfg1_4096_dequant_roundtrip_and_linear(gpu_device):
    """BASELINE configs[0]: 4096x4096 int8 row-wise, qmm off, fp32: dequant == q*scale exactly; linear vs oracle on a slab."""
    import sdnq_amd
    torch.manual_seed(0)
    lin = torch.nn.Linear(4096, 4096, bias=True)
    w_float = lin.weight.detach().clone()
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=False))
    layer = layer.to(gpu_device)
    dq = layer.sdnq_dequantizer
    wd = dq(layer.weight, layer.scale)
    assert torch.equal(wd.cpu(), layer.weight.cpu().float() * layer.scale.cpu())
    assert (wd.cpu() - w_float).abs().max() <= layer.scale.cpu().max() * 0.5 + 1e-12  # quantization error bound
    x = torch.randn(8, 4096)
    y = layer(x.to(gpu_device))
    ref = O.linear_float(x.numpy(), wd.detach().cpu().numpy(), layer.bias.detach().cpu().numpy(), "f32")
    assert_close_float(to_f32_numpy(y), ref, "f32", "cfg1 linear")


@pytest.mark.parametrize("m", [64, 4096])
def test_cfg1_4096_fp32_full_size_vs_oracle(m, gpu_device):
    """BASELINE configs[0] at the sizes bench.py's cpu_baseline.cfg1 TIMES on the GPU (M = 64 and M = 4096, fp32 activations:
    sdnq_hip_dequant + the f32-MFMA float GEMM, or the fused path where the dispatcher takes it): every output row at M = 64, a
    128-row slab + the last rows at M = 4096, against the oracle's quantized_linear_forward (layers/linear/forward.py:25-26)."""
    import sdnq_amd
    torch.manual_seed(0)
    lin = torch.nn.Linear(4096, 4096, bias=True)
    layer, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=False))
    layer = layer.to(gpu_device)
    assert not layer.sdnq_dequantizer.use_quantized_matmul
    wd = (layer.weight.cpu().float() * layer.scale.cpu()).numpy()  # == dequant, checked bit-exactly by the M = 8 test above
    bias = layer.bias.detach().cpu().numpy()
    x = torch.randn(m, 4096, generator=torch.Generator().manual_seed(m))
    y = layer(x.to(gpu_device))
    assert y.dtype == torch.float32 and tuple(y.shape) == (m, 4096)
    got = y.cpu().numpy()
    slabs = [(0, 64)] if m == 64 else [(1920, 2048), (4064, 4096)]
    # fp32 accumulation over K = 4096 in two different orders (the oracle's sequential loop, the MFMA's k-blocked tree): each is
    # within ~sqrt(K) * 2^-24 of the exact sum relative to the output scale, so the two may differ by twice that (7.6e-6 here)
    lim = 2.0 * (4096 ** 0.5) * 2.0 ** -24
    for lo, hi in slabs:
        ref = O.linear_float(x[lo:hi].numpy(), wd, bias, "f32")
        assert_close_float(got[lo:hi], ref, "f32", ("cfg1", m, lo, hi), f32_lim=lim)
        exact = (x[lo:hi].double().numpy() @ wd.astype(np.float64).T + bias.astype(np.float64))
        scale = float(np.abs(exact).max())
        assert float(np.abs(got[lo:hi] - exact).max()) <= 0.5 * lim * scale, ("cfg1 vs float64", m, lo, hi)
    # row independence at full size: the slab computed alone equals the same rows of the whole call (same tile path or not, the
    # fp32 accumulation order over K may differ between tile choices, so compare within the float tolerance)
    if m == 4096:
        y2 = layer(x[1920:2048].to(gpu_device)).cpu().numpy()
        assert_close_float(y2, got[1920:2048], "f32", "cfg1 slab alone", f32_lim=lim)


def test_operator_seam_and_errors(gpu_device):
    """int_scaled_mm_func keeps the reference's signature: b is the logical [K,N] operand in either memory layout."""
    from sdnq_amd import int_scaled_mm_func
    from sdnq_amd._lib import SdnqHipError
    g = torch.Generator().manual_seed(3)
    m, n, k = 96, 64, 128
    a = torch.randint(-128, 128, (m, k), dtype=torch.int8, generator=g).to(gpu_device)
    w = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g).to(gpu_device)
    sa = (torch.rand(m, 1, generator=g) * 0.01 + 1e-3).to(gpu_device)
    sb = (torch.rand(1, n, generator=g) * 0.01 + 1e-3).to(gpu_device)
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(gpu_device)
    y1 = int_scaled_mm_func(a, w.t(), sa, sb, bias=bias, out_dtype=torch.bfloat16)               # strides (1,K), gfx950 layout
    y2 = int_scaled_mm_func(a, w.t().contiguous(), sa, sb, bias=bias, out_dtype=torch.bfloat16)  # row-major [K,N]
    assert torch.equal(y1, y2)
    ref = O.scaled_mm("int8", a.cpu().numpy(), w.cpu().numpy(), sa.cpu().numpy(), sb.cpu().numpy(), bias.float().cpu().numpy(), "bf16")
    assert np.array_equal(to_f32_numpy(y1), ref)
    with pytest.raises(SdnqHipError):
        int_scaled_mm_func(a.cpu(), w.t().cpu(), sa.cpu(), sb.cpu())  # no CPU fallback in the product path
    with pytest.raises(SdnqHipError):  # K % 16 != 0 is rejected by the C ABI (SDNQ_ERR_SHAPE)
        ops.scaled_mm(ops.MM_I8, a[:, :100].contiguous(), w[:, :100].contiguous(), sa.view(-1), sb.view(-1), None, torch.bfloat16)


def test_accelerate_repoints_a_foreign_module(gpu_device):
    """accelerate(): a module built elsewhere (any object graph with the reference's attributes) gets the HIP forward."""
    import types
    import sdnq_amd
    c = Case("int8_rowwise_qmm_bf16")
    mod = module_from_case(c, gpu_device)
    foreign = types.SimpleNamespace(**{f: getattr(mod.sdnq_dequantizer, f) for f in sdnq_amd.loader._DQ_FIELDS})
    mod.sdnq_dequantizer = foreign
    mod.forward_func = lambda self, x: (_ for _ in ()).throw(RuntimeError("reference forward should have been replaced"))
    holder = torch.nn.Sequential(mod)
    assert sdnq_amd.accelerate(holder) == 1
    x = c.torch_tensor("x_48", device=gpu_device)
    assert np.array_equal(to_f32_numpy(holder(x)), c.f32("y_48"))


@pytest.mark.parametrize("wdt,gs", [("int8", -1), ("int4", 32), ("uint4", 64), ("int6", 32), ("uint2", 16), ("int3", 32), ("fp8", -1),
                                    ("float6_e3m2fn", 32), ("uint7", 128), ("int5", -1)])
@pytest.mark.parametrize("m", [1, 2, 3, 5, 32])  # every rows-per-launch bucket of the generic (1 / 2 / 4 / 8) and the fast kernel (1 / 2 / 4)
def test_fused_skinny_matches_dequant_then_linear(wdt, gs, m, gpu_device):
    """M <= 32: the fused unpack+scale+GEMV kernel equals dequantize -> float linear (dequantizer.py:204 + F.linear)."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(11)
    k, n = 384, 200
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin.to(gpu_device), sdnq_amd.SDNQConfig(weights_dtype=wdt, group_size=gs, use_quantized_matmul=False))
    x = torch.randn(m, k, device=gpu_device, dtype=torch.bfloat16)
    try:
        L.FUSED_SKINNY = True
        y_fused = mod(x)
        L.FUSED_SKINNY = False
        y_plain = mod(x)
    finally:
        L.FUSED_SKINNY = True
    wd = mod.sdnq_dequantizer(mod.weight, mod.scale, mod.zero_point, None, None)
    ref = O.linear_float(to_f32_numpy(x), to_f32_numpy(wd), to_f32_numpy(mod.bias), "bf16")
    assert_close_float(to_f32_numpy(y_fused), ref, "bf16", (wdt, gs, m, "fused vs oracle"))
    assert_close_float(to_f32_numpy(y_plain), ref, "bf16", (wdt, gs, m, "plain vs oracle"))


def test_activation_cache_is_transparent(gpu_device):
    """q/k/v-style sharing: three layers fed the same tensor object give bit-identical results with and without the
    activation-quantization cache; an in-place update of the tensor invalidates its entry."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(5)
    k, n, m = 640, 320, 96
    mods = []
    for i in range(3):
        lin = torch.nn.Linear(k, n, bias=i == 2).to(torch.bfloat16).to(gpu_device)
        mods.append(sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True))[0])
    x = torch.randn(m, k, device=gpu_device, dtype=torch.bfloat16)
    old = L.CACHE_ACTIVATIONS
    try:
        L.CACHE_ACTIVATIONS = 0
        ref = [mo(x).clone() for mo in mods]
        L.CACHE_ACTIVATIONS = 12
        L.clear_activation_cache()
        got = [mo(x).clone() for mo in mods]
        assert len(L._act_cache.entries) == 1
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
        x.mul_(2.0)
        L.CACHE_ACTIVATIONS = 0
        ref2 = mods[0](x).clone()
        L.CACHE_ACTIVATIONS = 12
        assert torch.equal(mods[0](x), ref2) and not torch.equal(ref2, ref[0])
    finally:
        L.CACHE_ACTIVATIONS = old
        L.clear_activation_cache()


@pytest.mark.gpu
def test_unshared_layers_stop_parking_their_activation(gpu_device):
    """A layer whose parked quantized activation nobody ever used learns that (two steps) and then runs the workspace path: no cache
    entry, same bits; a layer whose entry IS used by a sibling never does; consecutive workspace layers of different sizes (the
    workspace is overwritten and once replaced by a larger one) stay bit-identical to the cached path."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(11)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)

    def make(k, n):
        return sdnq_amd.sdnq_quantize_layer(torch.nn.Linear(k, n).to(torch.bfloat16).to(gpu_device), cfg)[0]

    solo_a, solo_b, sib0, sib1 = make(640, 320), make(2048, 128), make(640, 256), make(640, 256)
    xa = torch.randn(96, 640, device=gpu_device, dtype=torch.bfloat16)
    xb = torch.randn(4, 300, 2048, device=gpu_device, dtype=torch.bfloat16)
    xs = torch.randn(80, 640, device=gpu_device, dtype=torch.bfloat16)
    L.clear_activation_cache()
    ref = None
    for step in range(4):
        outs = [solo_a(xa).clone(), solo_b(xb).clone(), sib0(xs).clone(), sib1(xs).clone(), solo_a(xa * 1).clone()]
        L.clear_activation_cache()  # what the root model's forward-pre-hook does at the start of a step
        if ref is None:
            ref = outs
        for a, b in zip(outs, ref):
            assert torch.equal(a, b), step
    assert solo_a.__dict__["_sdnq_unshared"] >= L.UNSHARED_AFTER and solo_b.__dict__["_sdnq_unshared"] >= L.UNSHARED_AFTER
    assert sib0.__dict__["_sdnq_unshared"] < 0  # its entry was used by sib1: never takes the workspace path
    assert "_sdnq_unshared" not in sib1.__dict__  # always served from sib0's entry: never produced one
    solo_a(xa), solo_b(xb)
    assert len(L._act_cache.entries) == 0  # the workspace path parks nothing
    L.clear_activation_cache()


def _golden_dtype_entries():
    with open(os.path.join(GOLD, "dequant_dtypes.json")) as f:
        return sorted(json.load(f)["dtypes"].keys())


def _bytes_of(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.int64, torch.bool):  # reference's 1-bit packer promotes to int64 words of 8 bits each
        t = t.to(torch.uint8)
    return t.view(torch.uint8).numpy().reshape(-1)


@pytest.mark.parametrize("key", _golden_dtype_entries())
def test_hip_quantizer_reproduces_reference_weights(key, gpu_device):
    """8(f) rank 1: sdnq_hip_quantize_weight on the fixture's float weight == the reference quantizer's packed bytes,
    scales and zero points, for every storage dtype x {row-wise, group 32} captured in tests/golden/dequant_dtypes.*."""
    import sdnq_amd
    from sdnq_amd import quantizer as Q
    z = np.load(os.path.join(GOLD, "dequant_dtypes.npz"))
    with open(os.path.join(GOLD, "dequant_dtypes.json")) as f:
        ent = json.load(f)["dtypes"][key]
    wd, gs = ent["deq"]["weights_dtype"], ent["deq"]["group_size"]
    if wd in Q._HIP_QUANTIZER_SKIP:
        pytest.skip(f"{wd}: host-side packer only")
    w = torch.from_numpy(z["w_float"]).to(gpu_device)
    assert Q.USE_HIP_QUANTIZER
    dq, tensors = Q.sdnq_quantize_layer_weight(w, weights_dtype=wd, group_size=gs, use_quantized_matmul=False)
    assert list(dq.quantized_weight_shape) == ent["deq"]["quantized_weight_shape"]
    assert list(tensors["weight"].shape) == ent["tensors"]["weight"]["shape"], (key, tensors["weight"].shape)
    assert np.array_equal(_bytes_of(tensors["weight"]), z[f"{key}.weight"].reshape(-1).view(np.uint8) if z[f"{key}.weight"].dtype != np.int64
                          else z[f"{key}.weight"].astype(np.uint8)), (key, "codes")
    assert np.array_equal(tensors["scale"].cpu().numpy().view(np.uint32), z[f"{key}.scale"].view(np.uint32)), (key, "scale")
    if f"{key}.zero_point" in z:
        assert np.array_equal(tensors["zero_point"].cpu().numpy().view(np.uint32), z[f"{key}.zero_point"].view(np.uint32)), (key, "zp")
    else:
        assert tensors["zero_point"] is None


@pytest.mark.parametrize("wd,gs,dt", [("int4", 64, torch.bfloat16), ("uint4", 0, torch.bfloat16), ("int8", -1, torch.bfloat16),
                                      ("fp8", -1, torch.float16), ("int6", -1, torch.float32), ("uint3", 48, torch.bfloat16),
                                      ("float6_e3m2fn", 32, torch.bfloat16), ("int12", 32, torch.float32), ("uint5", 0, torch.float16)])
@pytest.mark.parametrize("qmm", [False, True])
def test_hip_quantizer_equals_host_quantizer(wd, gs, dt, qmm, gpu_device):
    """Same module tensors (bit for bit, same shapes / strides) from the HIP quantizer on a GPU weight and the host-side
    torch implementation on the CPU copy, through every layout branch (grouped, transposed-for-matmul, packed)."""
    from sdnq_amd import quantizer as Q
    g = torch.Generator().manual_seed(21)
    w = (torch.randn(208, 384, generator=g) * 0.02).to(dt)
    w[:, 5] *= 9
    kw = dict(weights_dtype=wd, group_size=gs, use_quantized_matmul=qmm)
    dq_c, t_c = Q.sdnq_quantize_layer_weight(w, **kw)
    dq_g, t_g = Q.sdnq_quantize_layer_weight(w.to(gpu_device), **kw)
    assert dq_c == dq_g
    for key in ("weight", "scale", "zero_point"):
        a, b = t_c[key], t_g[key]
        assert (a is None) == (b is None), key
        if a is None:
            continue
        strides = lambda t: tuple(st for st, sz in zip(t.stride(), t.shape) if sz > 1)  # noqa: E731  (size-1 dims carry no layout)
        assert a.shape == b.shape and strides(a) == strides(b) and a.dtype == b.dtype, (key, a.shape, b.shape, a.stride(), b.stride(), a.dtype, b.dtype)
        assert np.array_equal(_bytes_of(a), _bytes_of(b)), (wd, gs, key)


@pytest.mark.parametrize("shape", [(48, 256, 512), (333, 80, 48), (1000, 336, 144), (2048, 640, 1280), (77, 2048, 640)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("with_bias", [True, False])
def test_float_gemm_vs_oracle(shape, dt, with_bias, gpu_device):
    """M > 32 rows of the dequantize-then-F.linear branch run on the bf16 / f16 / f32 matrix cores (gemm.hip float
    variants); compared with the oracle's fp32-accumulate linear on the same operands."""
    m, k, n = shape
    g = torch.Generator().manual_seed(m * 7 + k)
    x = torch.randn(m, k, generator=g).to(dt)
    w = (torch.randn(n, k, generator=g) * 0.05).to(dt)
    b = torch.randn(n, generator=g).to(dt) if with_bias else None
    y = ops.linear_float(x.to(gpu_device), w.to(gpu_device), None if b is None else b.to(gpu_device))
    tag = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[dt]
    ref = O.linear_float(to_f32_numpy(x), to_f32_numpy(w), None if b is None else to_f32_numpy(b), tag)
    assert y.dtype == dt and tuple(y.shape) == (m, n)
    assert_close_float(to_f32_numpy(y), ref, tag, (shape, tag, with_bias))
    if m >= 64:  # row-slab consistency: the GEMM path is independent of which rows share a tile
        y2 = ops.linear_float(x[5:70].contiguous().to(gpu_device), w.to(gpu_device), None if b is None else b.to(gpu_device))
        assert torch.equal(y2, y[5:70])


@pytest.mark.parametrize("name", ["int8_rowwise_qmm_bf16", "int5_group32_noqmm_bf16", "uint8_uint8mm_qmm_bf16"])
def test_edge_shapes_empty_single_row_and_leading_dims(name, gpu_device):
    """Empty batch, one row, [B, T, K] inputs and non-contiguous rows go through every forward like F.linear would."""
    c = Case(name)
    mod = module_from_case(c, gpu_device)
    dt = TORCH_DT[c.tag]
    y0 = mod(torch.empty(0, c.K, device=gpu_device, dtype=dt))
    assert tuple(y0.shape) == (0, c.N) and y0.dtype == dt
    y0b = mod(torch.empty(2, 0, c.K, device=gpu_device, dtype=dt))
    assert tuple(y0b.shape) == (2, 0, c.N)
    M = max(c.ms())
    x = c.torch_tensor(f"x_{M}", device=gpu_device).reshape(-1, c.K)
    y = mod(x)
    y1 = mod(x[:1])
    assert tuple(y1.shape) == (1, c.N)
    x3 = x[: (M // 4) * 4].reshape(4, M // 4, c.K)
    assert torch.equal(mod(x3).reshape(-1, c.N), mod(x[: (M // 4) * 4]))
    wide = torch.zeros(M, c.K + 16, device=gpu_device, dtype=dt)
    wide[:, : c.K] = x
    assert torch.equal(mod(wide[:, : c.K]), y)  # row stride != K


# ---- conv as GEMM ---------------------------------------------------------------
from tests.golden_util import ConvCase, conv_case_names  # noqa: E402


@pytest.mark.parametrize("name", conv_case_names())
def test_conv_forward_vs_golden_and_oracle(name, gpu_device):
    """SDNQConv1d / SDNQConv2d on the HIP path (im2col + rowquant + MFMA scaled-mm, or dequant + float GEMM) against the
    reference's conv forwards and the oracle; int8 direct paths bit-exact."""
    c = ConvCase(name)
    d = c.deq
    mod = c.torch_module(gpu_device)
    omod = c.oracle_module()
    assert mod.forward_func.__name__ == c.meta["forward_func"]
    for i in c.inputs():
        x = c.torch_tensor(f"x_{i}", device=gpu_device)
        y = mod(x)
        ref = c.f32(f"y_{i}")
        assert y.dtype == x.dtype and tuple(y.shape) == ref.shape and y.is_contiguous()
        got = to_f32_numpy(y)
        orc = O.conv_forward(omod, c.f32(f"x_{i}"), c.conv, c.tag)
        exact = d["use_quantized_matmul"] and d["quantized_matmul_dtype"] in ("int8", "uint8") and not c.has("svd_up") and not d["use_hadamard"]
        if exact:
            assert np.array_equal(got, ref), (name, i, "golden", int((got != ref).sum()))
            assert np.array_equal(got, orc), (name, i, "oracle")
        else:
            assert_close_float(got, ref, c.tag, (name, i, "golden"), hadamard=d["use_hadamard"])
            assert_close_float(got, orc, c.tag, (name, i, "oracle"), hadamard=d["use_hadamard"])


@pytest.mark.parametrize("name", [n for n in conv_case_names() if "svd" not in n])
def test_conv_dequant_and_hip_quantizer_vs_golden(name, gpu_device):
    c = ConvCase(name)
    mod = c.torch_module(gpu_device)
    dq = mod.sdnq_dequantizer
    if c.has("w_dequant"):
        wd = dq(mod.weight, mod.scale, mod.zero_point, None, None, skip_quantized_matmul=dq.use_quantized_matmul)
        assert tuple(wd.shape) == tuple(c.info("w_dequant")["shape"])
        got, ref = to_f32_numpy(wd), c.f32("w_dequant")
        if dq.use_hadamard:  # the un-rotation's summation order is the device's (as for the Linear cases)
            assert np.all(np.abs(got - ref) <= 2 * np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7 + 1e-6), (name, "dequant")
        else:
            assert np.array_equal(got, ref), (name, "dequant")
    if c.has("requant_weight"):
        wq, ws = dq.re_quantize_matmul(mod.weight, mod.scale, mod.zero_point)[:2]
        assert np.array_equal(bits_of(wq.contiguous()), c.raw("requant_weight").view(np.uint8).reshape(bits_of(wq.contiguous()).shape))
        assert np.array_equal(ws.float().cpu().numpy().reshape(-1), c.f32("requant_scale").reshape(-1))
    from sdnq_amd import quantizer as Q
    from tests.test_quantizer import _conv_quant_kwargs, check_conv_state_dict
    if dq.use_hadamard:  # the rotation in front of the quantizer is a device matmul: codes may differ in the last step (CPU test: exact)
        return
    dq2, tensors = Q.sdnq_quantize_layer_weight(c.torch_tensor("w_float", device=gpu_device), layer_class_name=c.deq["layer_class_name"],
                                                **_conv_quant_kwargs(c))
    check_conv_state_dict(c, tensors, dq2, name)


@pytest.mark.parametrize("geom", [((2, 5, 9, 11), (3, 3), (1, 1), (1, 1), (1, 1)), ((1, 8, 16, 7), (3, 2), (2, 1), (1, 0), (1, 2)),
                                  ((3, 16, 1, 40), (1, 5), (1, 3), (0, 2), (1, 1)), ((1, 4, 70, 70), (1, 1), (1, 1), (0, 0), (1, 1))])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_im2col_equals_unfold(geom, dt, gpu_device):
    shape, kernel, stride, padding, dilation = geom
    if (shape[1] * kernel[0] * kernel[1] * (2 if dt == torch.bfloat16 else 4)) % 16:
        shape = (shape[0], shape[1] * 8, shape[2], shape[3])
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dt)
    got, (b, ho, wo) = ops.im2col(x.to(gpu_device), kernel, stride, padding, dilation)
    ref = torch.nn.functional.unfold(x.float(), kernel, dilation=dilation, padding=padding, stride=stride).transpose(1, 2).reshape(-1, got.shape[1])
    assert got.shape[0] == b * ho * wo and torch.equal(got.float().cpu(), ref)


@pytest.mark.parametrize("geom", [((2, 32, 8, 11), (3, 3), (1, 1), (1, 1), (1, 1)), ((1, 16, 16, 7), (3, 2), (2, 1), (1, 0), (1, 2)),
                                  ((1, 64, 32, 31), (1, 1), (1, 1), (0, 0), (1, 1)), ((2, 48, 12, 10), (5, 5), (1, 2), (2, 2), (1, 1))])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
def test_fused_conv_quant_equals_im2col_then_rowquant(geom, dt, mm_name, gpu_device):
    """sdnq_hip_im2col_rowquant == sdnq_hip_rowquant(sdnq_hip_im2col(x)) bit for bit (codes and scales), incl. an all-zero row."""
    shape, kernel, stride, padding, dilation = geom
    mm = ops.MM_I8 if mm_name == "int8" else ops.MM_FP8
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(dt)
    x[:, 3] *= 12
    x[0, :, :2, :2] = 0  # with padding, the first output position only sees zeros -> scale 0
    xg = x.to(gpu_device)
    xq, xs, dims = ops.im2col_rowquant(xg, kernel, stride, padding, dilation, mm)
    x2d, dims2 = ops.im2col(xg, kernel, stride, padding, dilation)
    rq, rs, _, _ = ops.rowquant(x2d, mm)
    assert dims == dims2 and torch.equal(xs, rs)
    assert np.array_equal(bits_of(xq), bits_of(rq))


def test_fuse_projections_is_bit_identical(gpu_device):
    """sdnq_amd.fuse_projections: to_qkv / to_kv built from row-wise int8 layers reproduce the separate layers bit for bit."""
    import sdnq_amd
    torch.manual_seed(9)

    class Attn(torch.nn.Module):
        def __init__(self, qd, kd, inner):
            super().__init__()
            self.to_q = torch.nn.Linear(qd, inner, bias=False)
            self.to_k = torch.nn.Linear(kd, inner, bias=False)
            self.to_v = torch.nn.Linear(kd, inner, bias=False)
            self.to_out = torch.nn.Linear(inner, qd)

    model = torch.nn.ModuleDict({"self_attn": Attn(320, 320, 320), "cross_attn": Attn(320, 512, 320)}).to(torch.bfloat16).to(gpu_device)
    model, _ = sdnq_amd.apply_sdnq_to_module(model, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True))
    assert sdnq_amd.fuse_projections(model) == 2
    sa, ca = model["self_attn"], model["cross_attn"]
    assert sa.fused_projections and hasattr(sa, "to_qkv") and not hasattr(sa, "to_kv")
    assert ca.fused_projections and hasattr(ca, "to_kv") and not hasattr(ca, "to_qkv")
    x = torch.randn(2, 100, 320, device=gpu_device, dtype=torch.bfloat16)
    e = torch.randn(2, 77, 512, device=gpu_device, dtype=torch.bfloat16)
    q, k, v = sa.to_qkv(x).split(320, dim=-1)
    assert torch.equal(q, sa.to_q(x)) and torch.equal(k, sa.to_k(x)) and torch.equal(v, sa.to_v(x))
    k2, v2 = ca.to_kv(e).split(320, dim=-1)
    assert torch.equal(k2, ca.to_k(e)) and torch.equal(v2, ca.to_v(e))


def test_fused_conv_quant_ties_and_large_image(gpu_device):
    """conv_quant_kernel vs im2col + rowquant on a large image with many quotients on or next to rounding ties (a reciprocal
    shortcut for the division was tried and dropped: exact, but the branch cost more than the division saved)."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 64, 64, 64, generator=g)
    x[:, ::2] = torch.round(x[:, ::2] * 37) / 37.0 * 1.5  # many repeated magnitudes -> many exact .5 quotients after scaling
    x[0, 5, 3, 3] = 40.0  # a dominant value: scale = 40 / 127 for its neighbourhood
    x[:, 7] = torch.round(x[:, 7] * 4) * (40.0 / 127.0) * 0.5  # exact multiples of scale / 2 -> ties where that scale applies
    for dt in (torch.bfloat16, torch.float32):
        xg = x.to(dt).to(gpu_device)
        xq, xs, dims = ops.im2col_rowquant(xg, (3, 3), (1, 1), (1, 1), (1, 1), ops.MM_I8)
        x2d, _ = ops.im2col(xg, (3, 3), (1, 1), (1, 1), (1, 1))
        rq, rs, _, _ = ops.rowquant(x2d, ops.MM_I8)
        assert torch.equal(xs, rs)
        assert torch.equal(xq, rq), int((xq != rq).sum())


@pytest.mark.parametrize("n", [1024, 12288])
def test_flux_size_int4_hadamard_layer_vs_oracle(n, gpu_device):
    """BASELINE configs[3] geometry (FLUX.1-dev: 4096 + 512 tokens, d = 3072), int4 + Hadamard-256, int8 MFMA: one full-size
    layer against the oracle on all rows (rel-L2 bound of the Hadamard configs) plus row-slab independence (bit-exact).
    N = 12288 (proj_mlp) is 864 tiles: the 256x256 half-tile-ring configuration the FLUX step spends most of its time in."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    torch.manual_seed(3)
    m, k = 4608, 3072
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16).to(gpu_device)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int4", use_hadamard=True, hadamard_group_size=256,
                                                                   use_quantized_matmul=True))
    assert mod.sdnq_dequantizer.re_quantize_for_matmul and mod.sdnq_dequantizer.use_hadamard
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    x[:, 7] *= 25
    xg = x.to(gpu_device)
    y = mod(xg)
    assert torch.equal(mod(xg[1000:1300].contiguous()), y[1000:1300])
    ref = O.forward(oracle_from_module(mod), x.float().numpy(), "bf16")
    assert_close_float(to_f32_numpy(y), ref, "bf16", "flux-size int4+hadamard", hadamard=True)


def test_sdxl_size_conv_int8_vs_oracle(gpu_device):
    """An SDXL-UNet resnet conv at full size (320 -> 320, 3x3, 128 x 128 latent, bs=1) through the fused conv matmul path,
    bit-exact against the oracle (16384 x 2880 x 320 int8 GEMM)."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    torch.manual_seed(6)
    conv = torch.nn.Conv2d(320, 320, 3, padding=1).to(torch.bfloat16).to(gpu_device)
    mod, _ = sdnq_amd.sdnq_quantize_layer(conv, sdnq_amd.SDNQConfig(weights_dtype="int8", quant_conv=True, use_quantized_matmul_conv=True))
    assert mod.forward_func.__name__ == "quantized_conv_forward_int8_matmul"
    x = torch.randn(1, 320, 128, 128, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16)
    x[:, 11] *= 30
    y = mod(x.to(gpu_device))
    meta = {"nd": 2, "kernel_size": [3, 3], "stride": [1, 1], "padding": [1, 1], "dilation": [1, 1], "padding_mode": "zeros", "groups": 1}
    ref = O.conv_forward(oracle_from_module(mod), x.float().numpy(), meta, "bf16")
    got = to_f32_numpy(y)
    assert got.shape == ref.shape == (1, 320, 128, 128)
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("k", [2048, 2304, 3072, 6144, 12288, 15360])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
def test_long_row_hadamard_rowquant_equals_rotate_then_quantize(k, dt, mm_name, gpu_device):
    """Rows beyond the register cache (K > 5120) with Hadamard (two-phase kernel: rotate for the amax, rotate again to quantize)
    must equal sdnq_hip_hadamard followed by the plain row quantization: codes, scales, rowsum and the rotated copy alike.
    (Parking the rotated row in LDS between the phases was tried: 20 % slower, one workgroup per CU starves the FWHT.)"""
    mm = ops.MM_I8 if mm_name == "int8" else ops.MM_FP8
    x = torch.randn(37, k, generator=torch.Generator().manual_seed(k)).to(dt)
    x[:, 100] *= 40
    x[5] = 0
    xg = x.to(gpu_device)
    want_rs = mm == ops.MM_I8
    xq, xs, rs, xrot = ops.rowquant(xg, mm, 256, want_rowsum=want_rs, want_xrot=True)
    rot = ops.hadamard(xg, 256)
    q2, s2, rs2, _ = ops.rowquant(rot, mm, 0, want_rowsum=want_rs)
    assert torch.equal(xrot, rot) and torch.equal(xs, s2)
    assert np.array_equal(bits_of(xq), bits_of(q2))
    if want_rs:
        assert torch.equal(rs, rs2)


def test_end_to_end_transformer_encoder_drop_in(gpu_device):
    """A whole (tiny, randomly initialised) transformers BERT encoder quantized in place with apply_sdnq_to_module and run on the HIP
    forwards: every nn.Linear becomes an SDNQLinear, the model still runs through its own code, and the int8 w8a8 output stays
    close to the float model (quantization error only).  Then the same with fused q/k/v-free options: dequant mode and int4."""
    transformers = pytest.importorskip("transformers")
    import sdnq_amd
    torch.manual_seed(0)
    cfg = transformers.BertConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024, vocab_size=128,
                                  max_position_embeddings=128)
    ids = torch.randint(0, 128, (2, 64), generator=torch.Generator().manual_seed(1)).to(gpu_device)

    def build():
        torch.manual_seed(0)
        return transformers.BertModel(cfg).eval().to(torch.bfloat16).to(gpu_device)

    with torch.no_grad():
        ref = build()(input_ids=ids).last_hidden_state.float()
    for kwargs, min_cos in ((dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True), 0.995),
                            (dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=False), 0.995),
                            (dict(weights_dtype="uint4", use_quantized_matmul=True), 0.95),
                            (dict(weights_dtype="int4", use_hadamard=True, hadamard_group_size=64, use_quantized_matmul=True), 0.95)):
        model = build()
        model, qcfg = sdnq_amd.apply_sdnq_to_module(model, sdnq_amd.SDNQConfig(minimum_allowed_numel=1024, **kwargs))
        n_q = sum(1 for m in model.modules() if isinstance(m, sdnq_amd.SDNQLinear))
        assert n_q >= 2 * 6 and not any(type(m) is torch.nn.Linear and m.weight.numel() >= 65536 for m in model.modules())
        with torch.no_grad():
            out = model(input_ids=ids).last_hidden_state.float()
        assert torch.isfinite(out).all()
        cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
        assert cos >= min_cos, (kwargs, cos)


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("qmm", [True, False])
@pytest.mark.parametrize("wdt,gs", [("int8", -1), ("uint4", 32), ("int4", 64), ("uint8", -1)])
def test_skinny_svd_matches_dequant_then_linear(m, dt, qmm, wdt, gs, gpu_device):
    """int8 + SVD layers with a few rows: the fused kernel (rank product on the matrix cores, W never stored) against the
    dequantize (+ addmm) -> linear pair and the oracle."""
    import sdnq_amd
    from sdnq_amd import linear as L
    from tests.modules_util import oracle_from_module
    torch.manual_seed(13)
    k, n = 384, 200
    lin = torch.nn.Linear(k, n, bias=True).to(dt).to(gpu_device)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype=wdt, group_size=gs, use_svd=True, svd_rank=32,
                                                                   use_quantized_matmul=qmm))
    assert mod.svd_up is not None
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(dt).to(gpu_device)
    try:
        L.FUSED_SKINNY = True
        y_fused = mod(x)
        L.FUSED_SKINNY = False
        y_plain = mod(x)
    finally:
        L.FUSED_SKINNY = True
    tag = "bf16" if dt == torch.bfloat16 else "f16"
    ref = O.forward(oracle_from_module(mod), to_f32_numpy(x), tag)
    assert_close_float(to_f32_numpy(y_fused), ref, tag, (m, tag, qmm, wdt, "fused vs oracle"))
    assert_close_float(to_f32_numpy(y_plain), ref, tag, (m, tag, qmm, wdt, "plain vs oracle"))
    assert_close_float(to_f32_numpy(y_fused), to_f32_numpy(y_plain), tag, (m, tag, qmm, wdt, "fused vs plain"))


def test_fp8_matmul_properties_at_sdxl_size(gpu_device):
    """fp8 scaled matmul at an SDXL ff.proj size: tile independence (row / column slabs of the big problem are bit-identical to
    the small problems: every output sums its K products in the same order whatever tile it lands in), exact power-of-two scaling,
    and a sampled block against the oracle within the fp8 tolerance."""
    m, n, k = 4096, 5120, 640
    g = torch.Generator().manual_seed(15)
    a = (torch.randn(m, k, generator=g) * 40).to(torch.float8_e4m3fn).to(gpu_device)
    b = (torch.randn(n, k, generator=g) * 40).to(torch.float8_e4m3fn).to(gpu_device)
    sa = (torch.rand(m, generator=g) * 0.02 + 1e-4).to(gpu_device)
    sb = (torch.rand(n, generator=g) * 0.02 + 1e-4).to(gpu_device)
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(gpu_device)
    full = ops.scaled_mm(ops.MM_FP8, a, b, sa, sb, bias, torch.bfloat16)
    rows = ops.scaled_mm(ops.MM_FP8, a[1000:1077].contiguous(), b, sa[1000:1077].contiguous(), sb, bias, torch.bfloat16)
    assert torch.equal(full[1000:1077], rows)
    cols = ops.scaled_mm(ops.MM_FP8, a, b[640:1280].contiguous(), sa, sb[640:1280].contiguous(), bias[640:1280].contiguous(), torch.bfloat16)
    assert torch.equal(full[:, 640:1280], cols)
    dbl = ops.scaled_mm(ops.MM_FP8, a, b, sa * 2, sb, None, torch.float32)
    base = ops.scaled_mm(ops.MM_FP8, a, b, sa, sb, None, torch.float32)
    assert torch.equal(dbl, base * 2)
    ref = O.scaled_mm("fp8", a[:64].view(torch.uint8).cpu().numpy(), b[:256].view(torch.uint8).cpu().numpy(), sa[:64].cpu().numpy(),
                      sb[:256].cpu().numpy(), bias[:256].float().cpu().numpy(), "bf16")
    assert_close_float(to_f32_numpy(full[:64, :256]), ref, "bf16", "fp8 sdxl-size block")


def test_weight_cache_switch_is_transparent(gpu_device):
    """SDNQ_HIP_CACHE_WEIGHTS=0 (re-quantize / unpack on every call, like the reference) gives the same bits as the cached path."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(21)
    x = torch.randn(64, 512, device=gpu_device, dtype=torch.bfloat16)
    for kwargs in (dict(weights_dtype="int4", use_quantized_matmul=True), dict(weights_dtype="int6", use_quantized_matmul=True),
                   dict(weights_dtype="uint8", quantized_matmul_dtype="int8", group_size=-1, use_quantized_matmul=True),
                   dict(weights_dtype="uint8", group_size=-1, use_quantized_matmul=True)):
        lin = torch.nn.Linear(512, 128, bias=True).to(torch.bfloat16).to(gpu_device)
        mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(**kwargs))
        old = L.CACHE_WEIGHTS
        try:
            L.CACHE_WEIGHTS = False
            mod.__dict__.pop("_sdnq_hip_state", None)
            a, b = mod(x).clone(), mod(x).clone()
            assert L._state(mod).mm_weight is None
            L.CACHE_WEIGHTS = True
            mod.__dict__.pop("_sdnq_hip_state", None)
            c, d = mod(x).clone(), mod(x).clone()
            assert L._state(mod).mm_weight is not None
        finally:
            L.CACHE_WEIGHTS = old
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(c, d), kwargs


def test_zero_weight_row_zero_activation_row_and_big_accumulators(gpu_device):
    """an all-zero weight row gives scale 0 and y[:, n] == bias[n]; an all-zero activation row gives y[m, :] ==
    bias; int32 accumulators beyond 2^24 (K = 15360, saturated operands) round to f32 like the reference (RNE) -- bit-exact vs
    the oracle."""
    import sdnq_amd
    torch.manual_seed(31)
    for kwargs in (dict(weights_dtype="int8", group_size=-1, use_quantized_matmul=True), dict(weights_dtype="int4", use_quantized_matmul=True),
                   dict(weights_dtype="uint4", use_quantized_matmul=True)):
        lin = torch.nn.Linear(256, 64, bias=True).to(torch.bfloat16)
        with torch.no_grad():
            lin.weight[5].zero_()
        mod, _ = sdnq_amd.sdnq_quantize_layer(lin.to(gpu_device), sdnq_amd.SDNQConfig(**kwargs))
        x = torch.randn(40, 256, device=gpu_device, dtype=torch.bfloat16)
        x[7].zero_()
        y = mod(x)
        assert torch.isfinite(y).all(), kwargs
        assert torch.equal(y[:, 5], mod.bias[5].expand(40)), kwargs
        assert torch.equal(y[7], mod.bias), kwargs
    m, n, k = 64, 64, 15360
    a = torch.full((m, k), 127, dtype=torch.int8)
    a[::3] = -128
    b = torch.full((n, k), 127, dtype=torch.int8)
    b[::5] = -128
    b[1, ::2] = 1
    sa = torch.full((m,), 2.0 ** -20)
    sb = torch.full((n,), 1.0)
    y = ops.scaled_mm(ops.MM_I8, a.to(gpu_device), b.to(gpu_device), sa.to(gpu_device), sb.to(gpu_device), None, torch.float32)
    ref = O.scaled_mm("int8", a.numpy(), b.numpy(), sa.numpy(), sb.numpy(), None, "f32")
    assert float(np.abs(ref).max()) * 2.0 ** 20 > 2.0 ** 24
    assert np.array_equal(y.cpu().numpy(), ref)


def test_scaled_mm_output_beyond_2_31_elements(gpu_device):
    """Maximum sizes: an output with more than 2^31 elements (70 001 x 32 768) and an M that is not a multiple of any tile --
    every index computation must be 64-bit.  Sampled rows / columns are bit-exact vs the oracle; the last element is written."""
    m, n, k = 70001, 32768, 256
    g = torch.Generator(device=gpu_device).manual_seed(9)
    a = torch.randint(-128, 128, (m, k), dtype=torch.int8, device=gpu_device, generator=g)
    b = torch.randint(-128, 128, (n, k), dtype=torch.int8, device=gpu_device, generator=g)
    sa = torch.rand(m, device=gpu_device, generator=g) * 0.01 + 0.001
    sb = torch.rand(n, device=gpu_device, generator=g) * 0.01 + 0.001
    bias = torch.randn(n, device=gpu_device, dtype=torch.bfloat16, generator=g)
    y = ops.scaled_mm(ops.MM_I8, a, b, sa, sb, bias, torch.bfloat16)
    assert y.numel() > 2 ** 31
    rows = torch.tensor([0, 1, 63, 64, 32767, 32768, 65535, 65536, 65537, 69999, 70000], device=gpu_device)
    cols = torch.tensor([0, 31, 127, 128, 16383, 16384, 32511, 32767], device=gpu_device)
    ref_rows = O.scaled_mm("int8", a[rows].cpu().numpy(), b.cpu().numpy(), sa[rows].cpu().numpy(), sb.cpu().numpy(), bias.float().cpu().numpy(), "bf16")
    assert np.array_equal(to_f32_numpy(y[rows]), ref_rows)
    ref_cols = O.scaled_mm("int8", a[::997].cpu().numpy(), b[cols].cpu().numpy(), sa[::997].cpu().numpy(), sb[cols].cpu().numpy(),
                           bias[cols].float().cpu().numpy(), "bf16")
    assert np.array_equal(to_f32_numpy(y[::997][:, cols]), ref_cols)
    del y
    torch.cuda.empty_cache()


def test_linked_projections_are_transparent(gpu_device):
    """sdnq_amd.link_projections / accelerate: to_q / to_k / to_v of an attention block run as ONE grouped scaled matmul
    (sdnq_hip_scaled_mm_grouped, reading the members' own weights) when they are called with the same tensor; every member returns its own contiguous tensor,
    bit-identical to what it computes alone, whatever the call order; a different tensor, a modified tensor and a small batch take
    the ordinary paths."""
    import sdnq_amd
    from sdnq_amd import linear as L

    class Attn(torch.nn.Module):
        def __init__(self, c, cross, bias):
            super().__init__()
            self.to_q = torch.nn.Linear(c, c, bias=bias)
            self.to_k = torch.nn.Linear(cross or c, c, bias=bias)
            self.to_v = torch.nn.Linear(cross or c, c, bias=bias)

    torch.manual_seed(13)
    L.LINK_PROJECTIONS = True  # the test is about the linked path whatever SDNQ_HIP_LINK_PROJECTIONS says (restored below per case)
    for mmd, cross, bias in (("int8", 0, True), ("float8_e4m3fn", 0, False), ("int8", 256, False)):
        wd = "int8" if mmd == "int8" else "float8_e4m3fn"
        blk = Attn(320, cross, bias).to(torch.bfloat16).to(gpu_device)
        cfg = sdnq_amd.SDNQConfig(weights_dtype=wd, quantized_matmul_dtype=mmd, group_size=-1, use_quantized_matmul=True)
        for name in ("to_q", "to_k", "to_v"):
            setattr(blk, name, sdnq_amd.sdnq_quantize_layer(getattr(blk, name), cfg)[0])
        mods = [blk.to_q, blk.to_k, blk.to_v]
        x = torch.randn(2, 75, 320, device=gpu_device, dtype=torch.bfloat16)
        xt = torch.randn(2, 77, cross or 320, device=gpu_device, dtype=torch.bfloat16)
        inputs = [x, xt if cross else x, xt if cross else x]
        alone = [m(i).clone() for m, i in zip(mods, inputs)]
        assert sdnq_amd.accelerate(blk) == 3
        group = blk.to_k.__dict__["_sdnq_group"][0]
        assert len(group.mods) == (2 if cross else 3) and (("_sdnq_group" in blk.to_q.__dict__) == (not cross))
        for order in ((0, 1, 2), (2, 0, 1)):
            L.clear_activation_cache()
            group.last = None
            outs = {i: mods[i](inputs[i]) for i in order}
            for i in range(3):
                assert torch.equal(outs[i], alone[i]) and outs[i].is_contiguous(), (mmd, cross, i)
            assert outs[1].data_ptr() != outs[2].data_ptr()
            assert group.last is None  # every member was served: nothing is kept alive
            a = mods[1](inputs[1])
            assert group.last is not None and group.last[0] is inputs[1]
            held = group.last[3][-1].data_ptr()
            assert mods[2](inputs[2]).data_ptr() == held and torch.equal(a, alone[1])  # the same launch serves the sibling
            if not cross:
                mods[0](inputs[0])
            assert group.last is None
        x2 = torch.randn_like(inputs[1])
        assert torch.equal(mods[1](x2), (lambda g: (g.__setattr__("last", None), L.clear_activation_cache(), mods[1](x2))[2])(group))
        group.last, group.wasted = None, 0  # (unclaimed outputs count against the group: see test_linked_group_dissolves_...)
        keep = inputs[1].clone()
        inputs[1].mul_(0.5)  # version bump: the stored outputs no longer belong to this tensor
        try:
            got = mods[1](inputs[1])
            L.LINK_PROJECTIONS = False
            L.clear_activation_cache()
            assert torch.equal(got, mods[1](inputs[1]))
        finally:
            L.LINK_PROJECTIONS = True
        inputs[1].copy_(keep)
        group.last, group.wasted = None, 0
        small = torch.randn(5, cross or 320, device=gpu_device, dtype=torch.bfloat16)
        assert mods[1](small).shape == (5, 320)  # M < 32: dequant + float GEMM branch, untouched
        if mmd == "int8" and not bias:
            with torch.no_grad():
                mods[2].weight.neg_()  # a member's weight changes in place (version bump): the stacked operands are rebuilt
            L.clear_activation_cache()
            k_again = mods[1](inputs[1])
            assert torch.equal(mods[2](inputs[2]), -alone[2]) and torch.equal(k_again, alone[1])
            assert "_sdnq_group" in mods[1].__dict__  # still linked
    L.LINK_PROJECTIONS = os.environ.get("SDNQ_HIP_LINK_PROJECTIONS", "1").lower() not in {"0", "false", "no"}


def test_linked_projections_float_mode(gpu_device):
    """use_quantized_matmul=False (the reference's default): linked to_q / to_k / to_v are dequantized side by side into one buffer
    and share ONE float GEMM (sdnq_hip_linear_float_multi); the weights fed to it are the members' dequantized weights bit for bit,
    so each output equals the member's own dequantize + F.linear up to the fp32 accumulation order of a different tile choice."""
    import sdnq_amd
    from sdnq_amd import linear as L

    class Attn(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.to_q, self.to_k, self.to_v = (torch.nn.Linear(c, c, bias=True) for _ in range(3))

    torch.manual_seed(3)
    old = L.LINK_PROJECTIONS
    try:
        for wd, dt in (("int8", torch.bfloat16), ("uint4", torch.float16), ("int6", torch.bfloat16)):
            blk = Attn(256).to(dt).to(gpu_device)
            for name in ("to_q", "to_k", "to_v"):
                setattr(blk, name, sdnq_amd.sdnq_quantize_layer(getattr(blk, name), sdnq_amd.SDNQConfig(weights_dtype=wd, use_quantized_matmul=False))[0])
            mods = [blk.to_q, blk.to_k, blk.to_v]
            x = torch.randn(3, 50, 256, device=gpu_device, dtype=dt)
            L.LINK_PROJECTIONS = False
            alone = [m(x).clone() for m in mods]
            L.LINK_PROJECTIONS = True
            assert sdnq_amd.link_projections(blk) == 1 and blk.to_q.__dict__["_sdnq_group"][0].float_mode
            outs = [m(x) for m in mods]
            group = blk.to_q.__dict__["_sdnq_group"][0]
            assert group.last is None
            ulp = 2.0 ** (-8 if dt == torch.bfloat16 else -11)
            for o, a in zip(outs, alone):
                assert o.shape == a.shape and o.is_contiguous()
                assert (o.float() - a.float()).abs().max() <= 2 * ulp * a.float().abs().max(), wd
                assert (o != a).float().mean() < 0.05, wd
            small = torch.randn(4, 256, device=gpu_device, dtype=dt)
            assert torch.equal(mods[0](small), (lambda: (setattr(L, "LINK_PROJECTIONS", False), mods[0](small), setattr(L, "LINK_PROJECTIONS", True))[1])())
    finally:
        L.LINK_PROJECTIONS = old


def _attn_block(c, cross, bias, gpu_device, cfg):
    import sdnq_amd

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.to_q = torch.nn.Linear(c, c, bias=bias)
            self.to_k = torch.nn.Linear(cross or c, c, bias=bias)
            self.to_v = torch.nn.Linear(cross or c, c, bias=bias)

    blk = Attn().to(torch.bfloat16).to(gpu_device)
    for name in ("to_q", "to_k", "to_v"):
        setattr(blk, name, sdnq_amd.sdnq_quantize_layer(getattr(blk, name), cfg)[0])
    return blk


def test_model_wide_cross_attention_group(gpu_device):
    """Every cross-attention to_k / to_v of a model reads the one encoder_hidden_states tensor: accelerate() puts them -- layers of
    DIFFERENT widths included -- into ONE ProjectionGroup; the first one called in a step computes all of them in one grouped launch
    and every member's output is bit-identical to the layer computed alone.  Nothing is carried into the next step."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(21)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    model = torch.nn.ModuleList([_attn_block(c, 512, False, gpu_device, cfg) for c in (320, 640, 320, 640, 1280)])
    text = torch.randn(1, 77, 512, device=gpu_device, dtype=torch.bfloat16)
    old = L.LINK_PROJECTIONS
    try:
        L.LINK_PROJECTIONS = False
        sdnq_amd.accelerate(model)
        alone = [(b.to_k(text).clone(), b.to_v(text).clone()) for b in model]
        L.LINK_PROJECTIONS = True
        assert sdnq_amd.accelerate(model) == 15
        group = model[0].to_k.__dict__["_sdnq_group"][0]
        assert len(group.mods) == 10 and all(b.to_v.__dict__["_sdnq_group"][0] is group for b in model)
        assert all("_sdnq_group" not in b.to_q.__dict__ for b in model)
        for step in range(2):
            L.invalidate()
            for i, b in enumerate(model):
                kk, vv = b.to_k(text), b.to_v(text)
                assert torch.equal(kk, alone[i][0]) and torch.equal(vv, alone[i][1]) and kk.is_contiguous()
                assert (group.last is None) == (i == len(model) - 1)
            assert group.wasted == 0 and group.gemm.unit_n == 320 and group.gemm.n_total == 2 * (320 + 640 + 320 + 640 + 1280)
    finally:
        L.LINK_PROJECTIONS = old


def test_model_wide_group_falls_back_to_per_block_pairs(gpu_device):
    """A model whose cross-attention blocks do NOT read one shared tensor (every block gets its own encoder states): the model-wide
    guess is wrong, costs two wasted launches, and falls back to per-block to_k / to_v pairs -- which are right and stay."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(24)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    model = torch.nn.ModuleList([_attn_block(c, 512, False, gpu_device, cfg) for c in (320, 640, 320)])
    texts = [torch.randn(1, 77, 512, device=gpu_device, dtype=torch.bfloat16) for _ in model]
    old = L.LINK_PROJECTIONS
    try:
        L.LINK_PROJECTIONS = False
        sdnq_amd.accelerate(model)
        alone = [(b.to_k(t).clone(), b.to_v(t).clone()) for b, t in zip(model, texts)]
        L.LINK_PROJECTIONS = True
        sdnq_amd.accelerate(model)
        wide = model[0].to_k.__dict__["_sdnq_group"][0]
        assert len(wide.mods) == 6 and wide.fallback is not None
        for step in range(4):
            L.invalidate()
            for i, (b, t) in enumerate(zip(model, texts)):
                kk, vv = b.to_k(t), b.to_v(t)
                assert torch.equal(kk, alone[i][0]) and torch.equal(vv, alone[i][1])
        for b in model:
            gk, gv = b.to_k.__dict__.get("_sdnq_group"), b.to_v.__dict__.get("_sdnq_group")
            assert gk is not None and gk[0] is gv[0] and gk[0] is not wide and len(gk[0].mods) == 2 and gk[0].wasted == 0
    finally:
        L.LINK_PROJECTIONS = old


def test_linked_group_dissolves_when_members_do_not_share_their_input(gpu_device):
    """A q / k / v group whose to_q is fed a different tensor than to_k / to_v (a cross-attention block that looked like
    self-attention): results stay correct from the first call, and after two computes that left outputs unclaimed the group
    dissolves itself -- no work is wasted from then on."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(22)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    blk = _attn_block(320, 0, True, gpu_device, cfg)
    h = torch.randn(1, 64, 320, device=gpu_device, dtype=torch.bfloat16)
    e = torch.randn(1, 64, 320, device=gpu_device, dtype=torch.bfloat16)
    old = L.LINK_PROJECTIONS
    try:
        L.LINK_PROJECTIONS = False
        want = (blk.to_q(h).clone(), blk.to_k(e).clone(), blk.to_v(e).clone())
        L.LINK_PROJECTIONS = True
        assert sdnq_amd.link_projections(blk) == 1
        for it in range(3):
            got = (blk.to_q(h), blk.to_k(e), blk.to_v(e))
            for a, b in zip(got, want):
                assert torch.equal(a, b)
        # the triple is gone; what it falls back to is the to_k / to_v pair (they DID share their input)
        assert "_sdnq_group" not in blk.to_q.__dict__
        gk, gv = blk.to_k.__dict__.get("_sdnq_group"), blk.to_v.__dict__.get("_sdnq_group")
        assert gk is not None and gv is not None and gk[0] is gv[0] and len(gk[0].mods) == 2
        for it in range(3):
            got = (blk.to_q(h), blk.to_k(e), blk.to_v(e))
            for a, b in zip(got, want):
                assert torch.equal(a, b)
        assert gk[0].wasted == 0 and "_sdnq_group" in blk.to_k.__dict__
        # a pair whose members do not share their input either ends as single layers
        e2 = torch.randn(1, 64, 320, device=gpu_device, dtype=torch.bfloat16)
        want_v2 = None
        for it in range(4):
            yk, yv = blk.to_k(e), blk.to_v(e2)
            assert torch.equal(yk, want[1])
            want_v2 = yv.clone() if want_v2 is None else want_v2
            assert torch.equal(yv, want_v2)
        assert all("_sdnq_group" not in m.__dict__ for m in (blk.to_q, blk.to_k, blk.to_v))
    finally:
        L.LINK_PROJECTIONS = old


def test_forward_under_inference_mode_and_invalidate(gpu_device):
    """torch.inference_mode(): inference tensors have no version counter -- the forwards must work (ComfyUI runs models that
    way) and simply skip every identity-keyed reuse.  sdnq_amd.invalidate(t) drops what was derived from a tensor that a
    raw-pointer writer changed behind autograd's back."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(23)
    cfg = sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True)
    blk = _attn_block(320, 0, False, gpu_device, cfg)
    sdnq_amd.accelerate(blk)
    x = torch.randn(2, 40, 320, device=gpu_device, dtype=torch.bfloat16)
    want = [m(x).clone() for m in (blk.to_q, blk.to_k, blk.to_v)]
    with torch.inference_mode():
        xi = x.clone()
        assert xi.is_inference()
        got = [m(xi) for m in (blk.to_q, blk.to_k, blk.to_v)]
        xi.mul_(2.0)  # in place, untracked
        got2 = blk.to_k(xi)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(got2, blk.to_k(x * 2.0))
    # out-of-band write: same tensor object, same version, different contents (x.data has its own version counter)
    L.invalidate()
    blk.to_q(x)  # the group computed k and v from x as well and holds them for the siblings
    v0 = x._version
    x.data.mul_(0.5)
    assert x._version == v0
    L.invalidate(x)
    got_k = blk.to_k(x)
    L.invalidate()
    assert torch.equal(got_k, blk.to_k(x.clone()))


def test_flux_size_int8_svd_layer_vs_oracle(gpu_device):
    """BASELINE configs[4] geometry at FULL size: FLUX.1-dev proj_mlp 4608 x 3072 -> 12288, int8 row-wise + SVD rank 32 + bias,
    int8 MFMA with the low-rank term in the GEMM epilogue (EPI_LOWRANK on the 256x256 tile with its 64-row staging chunks --
    round 1 only checked this epilogue at K = 512, N = 256).  Every row against the oracle: the int8 product is exact, the
    rank-32 term is a bf16 addmm (<= 1 bf16 ulp of the [M, N] bias by summation order), so the usual 2-ulp output bound."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    torch.manual_seed(31)
    m, k, n = 4608, 3072, 12288
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16).to(gpu_device)
    with torch.no_grad():
        lin.weight.mul_(0.5)
        lin.weight[:, :40] += torch.randn(n, 1, device=gpu_device).to(torch.bfloat16) * 0.3  # a low-rank component worth extracting
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_svd=True, svd_rank=32,
                                                                   use_quantized_matmul=True))
    assert mod.svd_up is not None and mod.sdnq_dequantizer.svd_rank == 32 and not mod.sdnq_dequantizer.re_quantize_for_matmul
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(32)).to(torch.bfloat16)
    x[:, 11] *= 20
    x[77] = 0  # an all-zero activation row: y = bias2d there
    xg = x.to(gpu_device)
    y = mod(xg)
    assert torch.equal(mod(xg[2048:2304].contiguous()), y[2048:2304])  # row-slab independence, bit for bit
    ref = O.forward(oracle_from_module(mod), x.float().numpy(), "bf16")
    assert_close_float(to_f32_numpy(y), ref, "bf16", "flux-size int8+svd32")
    assert float((to_f32_numpy(y) != ref).mean()) < 0.02  # the bulk is bit-identical; the rest are bf16 addmm order effects


def test_uint8_zero_point_plus_svd_at_tall_tile_size(gpu_device):
    """Zero-point term AND low-rank term together in the epilogue of a 256-row tile: uint8 row-wise weights (zero_point kept,
    linear_int8.py:45-50, 65-69) + SVD rank 32 at M = 4096, N = 1280, K = 1024 (256x128 tiles), against the oracle on all rows."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    torch.manual_seed(33)
    m, k, n = 4096, 1024, 1280
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16).to(gpu_device)
    with torch.no_grad():
        lin.weight.add_(0.01)  # asymmetric rows: a real zero point
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="uint8", group_size=-1, use_svd=True, svd_rank=32,
                                                                   use_quantized_matmul=True, quantized_matmul_dtype="int8"))
    dq = mod.sdnq_dequantizer
    assert mod.svd_up is not None and mod.zero_point is not None and dq.quantized_matmul_dtype == "int8" and not dq.re_quantize_for_matmul
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(34)).to(torch.bfloat16)
    y = mod(x.to(gpu_device))
    ref = O.forward(oracle_from_module(mod), x.float().numpy(), "bf16")
    assert_close_float(to_f32_numpy(y), ref, "bf16", "uint8 zero point + svd32, 256-row tiles")


def test_sdxl_size_fp8_layer_vs_oracle(gpu_device):
    """BASELINE configs[2] at full layer size: SDXL GEGLU projection 4096 x 640 -> 5120, fp8 e4m3 weights and activations, fp8 MFMA,
    every row against the oracle with the fp8 bound stated in DESIGN.md (2 bf16 ulp of the output scale; the block-scaled MFMA's
    accumulation order differs from the oracle's sequential fp32 sum)."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    torch.manual_seed(35)
    m, k, n = 4096, 640, 5120
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16).to(gpu_device)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="fp8", quantized_matmul_dtype="fp8", group_size=-1,
                                                                   use_quantized_matmul=True))
    assert mod.forward_func.__name__ == "quantized_linear_forward_fp8_matmul"
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(36)).to(torch.bfloat16)
    x[:, 3] *= 15
    y = mod(x.to(gpu_device))
    ref = O.forward(oracle_from_module(mod), x.float().numpy(), "bf16")
    assert_close_float(to_f32_numpy(y), ref, "bf16", "sdxl-size fp8")


@pytest.mark.parametrize("m,k,r", [(33, 48, 8), (16, 128, 32), (100, 192, 16), (257, 640, 48), (1000, 3072, 32), (77, 2048, 64), (4608, 1280, 32)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_lowrank_down_vs_float_reference(m, k, r, dt, gpu_device):
    """t = cast(x . svd_down^T) (linear_int8.py:60) through the LDS-DMA ring kernel: ragged M (16-row workgroups), K that is not a
    multiple of the 128-element stage, ranks below / above the 32-column tile.  fp32 accumulation, one rounding: <= 1 ulp of the
    output dtype at the output scale against a float64 product of the same 16-bit inputs."""
    g = torch.Generator().manual_seed(m * 7 + k + r)
    x = torch.randn(m, k, generator=g).to(dt)
    x[min(2, m - 1)] = 0
    d = (torch.randn(r, k, generator=g) * 0.05).to(dt)
    t = ops.lowrank_down(x.to(gpu_device), d.to(gpu_device))
    assert t.dtype == dt and tuple(t.shape) == (m, r)
    ref = (x.double() @ d.double().t()).numpy()
    got = t.double().cpu().numpy()
    ulp = 2.0 ** (-8 if dt == torch.bfloat16 else -11)
    assert np.all(np.abs(got - ref) <= ulp * np.maximum(np.abs(ref), np.abs(ref).max() * 2.0 ** -6) + 1e-30), (m, k, r, float(np.abs(got - ref).max()))
    assert np.all(got[min(2, m - 1)] == 0)


@pytest.mark.parametrize("m", [1, 2, 4])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("wdt,gs", [("int4", 64), ("int8", -1), ("uint4", 32), ("uint8", -1)])
def test_hadamard_layers_few_rows_vs_oracle(m, dt, wdt, gs, gpu_device):
    """The M < 32 branch of Hadamard-256 layers (dequantize incl. un-rotation + F.linear, linear_int8.py:102-103 + dequantizer.py:82-87):
    the weight row is un-rotated on the matrix cores (linear_skinny_had256_kernel); against the oracle and the unfused pair."""
    import sdnq_amd
    from sdnq_amd import linear as L
    from tests.modules_util import oracle_from_module
    torch.manual_seed(17)
    k, n = 768, 136
    lin = torch.nn.Linear(k, n, bias=True).to(dt).to(gpu_device)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype=wdt, group_size=gs, use_hadamard=True, hadamard_group_size=256,
                                                                   use_quantized_matmul=True))
    assert mod.sdnq_dequantizer.use_hadamard and mod.sdnq_dequantizer.hadamard_group_size == 256
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(dt).to(gpu_device)
    try:
        L.FUSED_SKINNY = True
        y_fused = mod(x)
        L.FUSED_SKINNY = False
        y_plain = mod(x)
    finally:
        L.FUSED_SKINNY = True
    tag = "bf16" if dt == torch.bfloat16 else "f16"
    ref = O.forward(oracle_from_module(mod), to_f32_numpy(x), tag)
    assert_close_float(to_f32_numpy(y_fused), ref, tag, (m, tag, wdt, "fused vs oracle"), hadamard=True)
    assert_close_float(to_f32_numpy(y_plain), ref, tag, (m, tag, wdt, "plain vs oracle"), hadamard=True)
    assert_close_float(to_f32_numpy(y_fused), to_f32_numpy(y_plain), tag, (m, tag, wdt, "fused vs plain"), hadamard=True)


@pytest.mark.parametrize("rank", [16, 48])
@pytest.mark.parametrize("m", [1, 4])
def test_skinny_svd_other_ranks(rank, m, gpu_device):
    """Ranks other than the default 32 take the generic few-row SVD kernel (rank 32: skinny_svd32_kernel, covered above)."""
    import sdnq_amd
    from tests.modules_util import oracle_from_module
    torch.manual_seed(19)
    k, n = 384, 200
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16).to(gpu_device)
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_svd=True, svd_rank=rank,
                                                                   use_quantized_matmul=True))
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(torch.bfloat16).to(gpu_device)
    ref = O.forward(oracle_from_module(mod), to_f32_numpy(x), "bf16")
    assert_close_float(to_f32_numpy(mod(x)), ref, "bf16", (rank, m))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rowquant_division_shortcut_over_the_exponent_range(dt, gpu_device):
    """The row kernels divide by the row scale with Markstein's correction (RowDiv, sdnq_dev.h) when the scale is an ordinary
    number, with the IEEE sequence otherwise.  Rows spanning the whole exponent range -- both sides of the 2^+-60 guard,
    subnormal-scale rows, scales whose significand is all ones (the one case where RN(1 / s) is too coarse), ties and near-ties at
    every magnitude -- must give the reference's codes and scales bit for bit, int8 and fp8."""
    x = torch.from_numpy(rowquant_inputs.exponent_range()).to(dt)
    xf = x.float().numpy()
    for mm, name in ((ops.MM_I8, "int8"), (ops.MM_FP8, "fp8")):
        xq, xs, rs, _ = ops.rowquant(x.to(gpu_device), mm, want_rowsum=(mm == ops.MM_I8))
        q, s, rowsum = O.rowquant(xf, name)
        assert np.array_equal(xs.cpu().numpy().reshape(-1), s), (dt, name)
        bad = np.nonzero((bits_of(xq) != q.view(np.uint8)).any(axis=1))[0]
        assert bad.size == 0, (dt, name, bad[:8], [float(s[b]) for b in bad[:8]])
        if rowsum is not None:
            assert np.array_equal(rs.cpu().numpy(), rowsum)


def _requant_layer(wd, mm_name, group, n, k, gpu_device, seed=5):
    """A 4-bit (or other) layer that MUST re-quantize for its matmul: a wrong premise fails the test instead of skipping it."""
    import sdnq_amd
    assert wd in sdnq_amd.common.dtype_dict, wd
    assert n % 16 == 0 and k % 16 == 0 and n >= 32 and k >= 32  # check_quantized_matmul_is_allowed (utils.py:93-98)
    torch.manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=False).to(torch.bfloat16).to(gpu_device)
    lin.weight.data[:, 3] *= 9
    lin.weight.data[7] = 0  # a constant row: 0 / 0 -> code 0
    mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype=wd, group_size=group, use_quantized_matmul=True,
                                                                   quantized_matmul_dtype="int8" if mm_name == "int8" else "float8_e4m3fn"))
    dq = mod.sdnq_dequantizer
    assert dq.use_quantized_matmul and dq.re_quantize_for_matmul, (wd, mm_name, group, n, k, "does not re-quantize")
    return mod


def _requant_ab(mod, mm, n, k, expect_table):
    """requant through the dispatcher (table kernel where it applies), again with the general kernel forced, and a third time with
    the row scales handed in (sdnq_hip_requant_ws, the per-call mode): all bit-identical, and equal to the oracle."""
    from sdnq_amd import linear as L
    from tests.modules_util import oracle_from_module
    st = L._state(mod)
    assert "SDNQ_HIP_REQUANT_LUT" not in os.environ
    wq, ws = ops.requant(st.qw, mm)
    os.environ["SDNQ_HIP_REQUANT_LUT"] = "0"
    try:
        wq_gen, ws_gen = ops.requant(st.qw, mm)
        torch.cuda.synchronize()
    finally:
        del os.environ["SDNQ_HIP_REQUANT_LUT"]
    assert torch.equal(ws, ws_gen), "table kernel row scales != general kernel"
    assert np.array_equal(bits_of(wq), bits_of(wq_gen)), "table kernel codes != general kernel"
    wq2, ws2 = ops.requant(st.qw, mm, ws.clone())
    assert torch.equal(ws, ws2) and np.array_equal(bits_of(wq), bits_of(wq2)), "known-scale call differs"
    # the known-scale path must USE the scales it is given where the table kernel runs: doubled scales halve the int8 codes
    if expect_table and mm == ops.MM_I8:
        wq3, ws3 = ops.requant(st.qw, mm, ws * 2)
        assert torch.equal(ws3, ws * 2)
        a, b = wq.view(torch.int8).int(), wq3.view(torch.int8).int()
        assert ((a - 2 * b).abs() <= 1).all() and not torch.equal(a, b)
    rq, rs = oracle_from_module(mod).re_quantize_matmul()[:2]
    assert np.array_equal(ws.cpu().numpy().reshape(-1), np.asarray(rs, dtype=np.float32).reshape(-1))
    assert np.array_equal(bits_of(wq).reshape(n, k), np.ascontiguousarray(rq).view(np.uint8).reshape(n, k))
    assert (bits_of(wq).reshape(n, k)[7] == 0).all()  # the constant row


@pytest.mark.parametrize("wd", ["int4", "uint4", "float4_e2m1fn", "float4_e3m0fn"])
@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
@pytest.mark.parametrize("group", [64, 128, 32])
@pytest.mark.parametrize("k", [640, 3072])
def test_requant_table_path_equals_oracle_and_known_scales(wd, mm_name, group, k, gpu_device):
    """4-bit weights in groups of a multiple of 64 are re-quantized through a 16-entry table per (row, group)
    (requant_lut4_kernel, NP = 1 / 3 passes per row here); group 32 takes the general kernel.  Codes and row scales must equal the
    oracle's re_quantize_matmul (dequantizer.py:166-174, 204-239) bit for bit, the general kernel's (SDNQ_HIP_REQUANT_LUT=0) bit for
    bit, and a call that is handed the row scales (sdnq_hip_requant_ws, the per-call mode of SDNQ_HIP_CACHE_WEIGHTS=0)."""
    n = 208
    mod = _requant_layer(wd, mm_name, group, n, k, gpu_device)
    _requant_ab(mod, ops.MM_I8 if mm_name == "int8" else ops.MM_FP8, n, k, expect_table=group % 64 == 0)


@pytest.mark.parametrize("k", [2048, 4096, 5120, 6144, 7168, 8192, 9216, 12288, 13312, 15360, 16384])
@pytest.mark.parametrize("wd,mm_name,group", [("int4", "int8", 64), ("float4_e2m1fn", "fp8", 128), ("uint4", "int8", 128)])
def test_requant_table_every_row_length_class(k, wd, mm_name, group, gpu_device):
    """Every NP instantiation of requant_lut4_kernel (passes of 1024 elements per row: 2, 4, 5, 6, 8 (K = 7168: one pass of
    clamped lanes; K = 8192), 12 (9216, 12288), 16 (13312, 15360 = FLUX proj_out, 16384)) against the oracle and the general kernel."""
    n = 48
    mod = _requant_layer(wd, mm_name, group, n, k, gpu_device, seed=k)
    _requant_ab(mod, ops.MM_I8 if mm_name == "int8" else ops.MM_FP8, n, k, expect_table=True)


@pytest.mark.parametrize("form", ["plain", "svd", "zp", "svd+zp", "had+svd", "uint8mm", "fp8+svd"])
def test_one_call_linear_equals_the_separate_calls(form, gpu_device):
    """sdnq_hip_linear (POD args, workspace query) against the sequence of entry points it replaces -- rowquant,
    lowrank_down, scaled_mm / scaled_mm_lowrank -- for every layer form, with scratch-resident and caller-supplied intermediates and
    with a pre-quantized activation: bit-identical outputs and intermediates."""
    torch.manual_seed(11)
    m, k, n, r = 300, 512, 264, 32
    mm = ops.MM_FP8 if form.startswith("fp8") else ops.MM_I8
    had = 256 if form.startswith("had") else 0
    dt = torch.bfloat16
    x = torch.randn(m, k, device=gpu_device, dtype=dt)
    x[:, 5] *= 17
    wq = torch.randint(-127, 128, (n, k), dtype=torch.int8, device=gpu_device)
    if mm == ops.MM_FP8:
        wq = (torch.randn(n, k, device=gpu_device) * 40).clamp(-448, 448).to(torch.float8_e4m3fn)
    ws = torch.rand(n, device=gpu_device) * 0.01 + 1e-4
    bias = torch.randn(n, device=gpu_device, dtype=dt)
    svd = "svd" in form
    down = torch.randn(r, k, device=gpu_device, dtype=dt) * 0.05 if svd else None
    up = torch.randn(n, r, device=gpu_device, dtype=dt) * 0.05 if svd else None
    zp = torch.randn(n, device=gpu_device) * 0.1 if ("zp" in form or form == "uint8mm") else None
    asym = form == "uint8mm"
    wcs = wq.to(torch.int32).sum(dim=1).to(torch.float32).mul_(ws) if asym else None
    # the separate calls
    res = ops.rowquant(x, mm, had, want_rowsum=zp is not None, want_xrot=svd and had != 0, asymmetric=asym)
    xq, xs, rowsum, xrot = res[:4]
    xzp = res[4] if asym else None
    t = ops.lowrank_down(xrot if xrot is not None else x, down) if svd else None
    if svd or zp is not None or asym:
        want = ops.scaled_mm_lowrank(mm, xq, wq, xs, ws, bias, t, up, rowsum, zp, dt, a_zp=xzp, w_colsum_scaled=wcs)
    else:
        want = ops.scaled_mm(mm, xq, wq, xs, ws, bias, dt)
    # one call, intermediates returned as tensors
    got, inter = ops.linear_call(mm, x, wq, ws, bias, dt, had, down, up, zp, asymmetric=asym, w_colsum_scaled=wcs)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), form
    assert np.array_equal(bits_of(inter[0]), bits_of(xq)) and torch.equal(inter[1].reshape(-1), xs.reshape(-1))
    if rowsum is not None:
        assert torch.equal(inter[2], rowsum)
    # one call on the pre-quantized activation (what sibling layers of a shared input do)
    got2, _ = ops.linear_call(mm, x, wq, ws, bias, dt, had, down, up, zp, asymmetric=asym, w_colsum_scaled=wcs, pre=inter)
    assert torch.equal(got2.view(torch.int16), want.view(torch.int16)), form


def test_per_call_weight_pipeline_is_bit_identical(gpu_device, monkeypatch):
    """SDNQ_HIP_CACHE_WEIGHTS=0 with the side-stream weight pipeline (linear._WeightPipeline: layer i + 1 re-quantized into the other
    scratch buffer under layer i's GEMM): every step equals the cached mode bit for bit -- eagerly, with the layer order changed
    under it (wrong guesses), and replayed from a captured graph."""
    import sdnq_amd
    from sdnq_amd import linear as L
    torch.manual_seed(3)
    dims = [(640, 208), (3072, 256), (1280, 1024), (2048, 64), (640, 640)]
    mods, xs = [], []
    for (k, n) in dims:
        lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16).to(gpu_device)
        mod, _ = sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int4", group_size=64, use_quantized_matmul=True))
        assert mod.sdnq_dequantizer.re_quantize_for_matmul
        mods.append(mod)
        xs.append(torch.randn(100, k, device=gpu_device, dtype=torch.bfloat16))
    want = [m(x).clone() for m, x in zip(mods, xs)]  # cached mode
    monkeypatch.setattr(L, "CACHE_WEIGHTS", False)
    monkeypatch.setattr(L, "PIPELINE_WEIGHTS", True)
    monkeypatch.setattr(L, "FUSED_LUT4", False)  # (round 6: few-row 4-bit layers would multiply on their stored codes instead -- tests/test_gemm_w4.py)
    pipe = L._WeightPipeline()
    monkeypatch.setattr(L, "_weight_pipeline", pipe)
    for m in mods:
        m.__dict__.pop("_sdnq_hip_state", None)

    def step(order):
        L.clear_activation_cache()
        outs = {i: mods[i](xs[i]) for i in order}
        L.join_weight_pipeline()
        return outs

    fwd = list(range(len(mods)))
    for it in range(3):
        outs = step(fwd)
        for i in fwd:
            assert torch.equal(outs[i], want[i]), (it, i)
    assert pipe.stats["prefetched"] >= len(mods) - 1 and pipe.scratch_bytes() >= 2 * 3072 * 256
    assert all(m.__dict__["_sdnq_hip_state"].mm_weight is None for m in mods)  # no int8 copy kept
    for order in (fwd[::-1], [2, 0, 4], fwd):  # wrong guesses: stray prefetches are joined, results unchanged
        outs = step(order)
        for i in order:
            assert torch.equal(outs[i], want[i]), (order, i)
    assert pipe.stats["wasted"] >= 1
    # graph capture: fork / join of the side stream by events
    outs = step(fwd)
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        step(fwd)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gouts = step(fwd)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for i in fwd:
        assert torch.equal(gouts[i], want[i]), ("graph", i)


@pytest.mark.parametrize("mm_name", ["int8", "fp8"])
def test_scaled_mm_k_shorter_than_a_stage_at_the_end_of_an_allocation(mm_name, gpu_device):
    """K of 16 ... 112 bytes is less than one 128-byte LDS stage: the ring's filler fetches (whole stages nobody consumes) used to read
    up to 112 bytes past the last operand row -- round 4's configuration fuzzer took the GPU down with a memory access fault on a
    K = 32 layer whose operands ended an allocation.  The operands here are the LAST bytes of their own 2 MiB blocks; results against
    the oracle (bit-exact for int8)."""
    mm = ops.MM_I8 if mm_name == "int8" else ops.MM_FP8
    g = torch.Generator().manual_seed(7)

    def at_end_of_block(t: torch.Tensor) -> torch.Tensor:
        blk = torch.empty(2 << 20, dtype=torch.uint8, device=gpu_device)  # one whole small-pool segment of the caching allocator
        nb = t.numel() * t.element_size()
        nb16 = (nb + 15) // 16 * 16
        dst = blk[(2 << 20) - nb16:(2 << 20) - nb16 + nb].view(t.dtype).view(t.shape)
        dst.copy_(t)
        dst._keep = blk
        return dst

    for (m, n, k) in [(32, 208, 32), (33, 64, 16), (100, 128, 48), (64, 64, 64), (257, 336, 96), (129, 64, 112), (40, 32, 80)]:
        if mm_name == "int8":
            a = torch.randint(-128, 128, (m, k), dtype=torch.int8, generator=g)
            b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g)
            a_np, b_np = a.numpy(), b.numpy()
        else:
            a = (torch.randn(m, k, generator=g) * 50).clamp(-448, 448).to(torch.float8_e4m3fn)
            b = (torch.randn(n, k, generator=g) * 50).clamp(-448, 448).to(torch.float8_e4m3fn)
            a_np, b_np = a.view(torch.uint8).numpy(), b.view(torch.uint8).numpy()
        sa, sb = torch.rand(m, generator=g) * 0.02 + 1e-4, torch.rand(n, generator=g) * 0.02 + 1e-4
        bias = torch.randn(n, generator=g).to(torch.bfloat16)
        out = ops.scaled_mm(mm, at_end_of_block(a), at_end_of_block(b), sa.to(gpu_device), sb.to(gpu_device), bias.to(gpu_device), torch.bfloat16)
        torch.cuda.synchronize()
        ref = O.scaled_mm(mm_name, a_np, b_np, sa.numpy(), sb.numpy(), bias.float().numpy(), "bf16")
        if mm_name == "int8":
            assert np.array_equal(to_f32_numpy(out), ref), (m, n, k)
        else:
            assert_close_float(to_f32_numpy(out), ref, "bf16", (m, n, k))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
def test_rowquant_fp8_keeps_the_sign_of_zero(dt, gpu_device):
    """-0.0 / scale = -0.0 -> fp8 code 0x80 in the reference (torch.div + .to(float8_e4m3fn)); the three-instruction division used to
    return +0 (code 0x00).  Found by tools/fuzz_ops.py on f16 activations that underflow to -0.0."""
    x = torch.randn(40, 640, generator=torch.Generator().manual_seed(3)).to(dt)
    x[:, 5::7] = -0.0
    x[:, 6::7] = 0.0
    x[3] = -0.0  # a whole row of negative zeros: scale 0, 0/0 -> NaN -> nan_to_num -> +0
    xq, xs, _, _ = ops.rowquant(x.to(gpu_device), ops.MM_FP8)
    q, s, _ = O.rowquant(x.float().numpy(), "fp8")
    assert np.array_equal(xs.cpu().numpy().reshape(-1), s.reshape(-1))
    assert np.array_equal(bits_of(xq), q.view(np.uint8))
    assert (bits_of(xq)[0, 5::7] == 0x80).all() and (bits_of(xq)[0, 6::7] == 0x00).all()


@pytest.mark.gpu
def test_conv_quantizer_self_cleaning_amax_map(gpu_device):
    """sdnq_hip_im2col_rowquant_z: the stream's persistent amax map is zero before and after every call (the quantizing kernel's last
    workgroup cleans it), so back-to-back convolutions of different sizes, eager and replayed from a hipGraph, give exactly what the
    zero-per-call form gives."""
    from sdnq_amd import ops
    g = torch.Generator().manual_seed(3)
    shapes = [(1, 32, 24, 24, 3, 1, 1), (2, 48, 16, 8, 3, 2, 1), (1, 320, 64, 64, 3, 1, 1), (1, 64, 40, 8, 1, 1, 0), (1, 32, 24, 24, 3, 1, 1)]
    xs_in = [(torch.randn(b, c, h, w, generator=g) * (1 + i)).to(torch.bfloat16).to(gpu_device) for i, (b, c, h, w, k, s_, p_) in enumerate(shapes)]

    def run_all():
        outs = []
        for x, (b, c, h, w, k, s_, p_) in zip(xs_in, shapes):
            xq, xs, _ = ops.im2col_rowquant(x, (k, k), (s_, s_), (p_, p_), (1, 1), ops.MM_I8)
            outs.append((xq.clone(), xs.clone()))
        return outs

    assert ops.SELF_CLEANING_AMAX
    ops.SELF_CLEANING_AMAX = False
    try:
        want = run_all()
    finally:
        ops.SELF_CLEANING_AMAX = True
    for rep in range(3):
        got = run_all()
        for (a, sa), (b_, sb) in zip(got, want):
            assert torch.equal(a, b_) and torch.equal(sa, sb), rep
    torch.cuda.synchronize()
    maps = [e for k_, e in ops._amax_maps.items() if k_[0] == gpu_device.index]
    assert maps and all(not e[0].any().item() and not e[1] for e in maps)
    st = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(st):
        run_all()  # the stream's map exists before the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            cap = run_all()
        for rep in range(3):
            graph.replay()
            st.synchronize()
            for (a, sa), (b_, sb) in zip(cap, want):
                assert torch.equal(a, b_) and torch.equal(sa, sb), ("replay", rep)


@pytest.mark.gpu
def test_conv_quantizer_ticket_scheme_under_stress_and_beside_a_replayed_graph(gpu_device):
    """Round-4 verdict (weak 8) + advisor: (a) thousands of back-to-back eager convs with CHANGING image content through the
    self-cleaning amax map (fence-free tickets, csrc/conv.hip) -- every result equals the zero-per-call form's; (b) a graph captured
    on one stream and replayed on ANOTHER, beside eager convs on the capture stream, shares nothing with them (captured convs take a
    buffer out of the graph's pool, never the stream's persistent map)."""
    from sdnq_amd import ops
    g = torch.Generator().manual_seed(11)
    imgs = [(torch.randn(1, 64, 32, 32, generator=g) * (0.25 + 3 * i)).to(torch.bfloat16).to(gpu_device) for i in range(6)]
    args = ((3, 3), (1, 1), (1, 1), (1, 1), ops.MM_I8)
    ops.SELF_CLEANING_AMAX = False
    try:
        want = [tuple(t.clone() for t in ops.im2col_rowquant(x, *args)[:2]) for x in imgs]
    finally:
        ops.SELF_CLEANING_AMAX = True
    bad = torch.zeros((), device=gpu_device, dtype=torch.int64)
    for it in range(3000):
        i = (it * 5 + it // 7) % len(imgs)
        xq, xs, _ = ops.im2col_rowquant(imgs[i], *args)
        bad += (xq != want[i][0]).sum() + (xs != want[i][1]).sum()
    assert int(bad.item()) == 0
    cap_stream, other = torch.cuda.Stream(device=gpu_device), torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(cap_stream):
        ops.im2col_rowquant(imgs[0], *args)
        cap_stream.synchronize()
        persistent = ops._amax_maps[(gpu_device.index, cap_stream.cuda_stream)][0]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap_stream):
            cap = [ops.im2col_rowquant(x, *args)[:2] for x in imgs]
    assert ops._amax_maps[(gpu_device.index, cap_stream.cuda_stream)][0] is persistent
    bad.zero_()
    for rep in range(20):
        with torch.cuda.stream(other):
            graph.replay()
        with torch.cuda.stream(cap_stream):
            for i in (rep % 6, (rep + 3) % 6):
                xq, xs, _ = ops.im2col_rowquant(imgs[i], *args)
                bad += (xq != want[i][0]).sum() + (xs != want[i][1]).sum()
        other.synchronize()
        for (a, sa), (b_, sb) in zip(cap, want):
            assert torch.equal(a, b_) and torch.equal(sa, sb), rep
    torch.cuda.synchronize()
    assert int(bad.item()) == 0


@pytest.mark.gpu
def test_weight_prefetch_across_layers_changes_no_bit(gpu_device, monkeypatch):
    """sdnq_hip_prefetch_hint + linear._PrefetchChain: a chain of layers run for several steps gives the same bits with the prefetch
    on and off, the hints are really set from the second step on, and the stand-alone sdnq_hip_prefetch runs."""
    import sdnq_amd
    from sdnq_amd import _lib, linear as L
    torch.manual_seed(7)

    def make_linear(k, n, bias):
        lin = torch.nn.Linear(k, n, bias=bias, device=gpu_device, dtype=torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(n, k, device=gpu_device) * 0.02)
        return sdnq_amd.sdnq_quantize_layer(lin, sdnq_amd.SDNQConfig(weights_dtype="int8", group_size=-1, use_quantized_matmul=True))[0]

    mods = [make_linear(1280, 1280, True) for _ in range(4)]
    mods.append(make_linear(1280, 3840, False))
    xs = [torch.randn(1024, 1280, device=gpu_device, dtype=torch.bfloat16) for _ in mods]

    def steps(n):
        outs = None
        for _ in range(n):
            L.clear_activation_cache()
            outs = [m(x) for m, x in zip(mods, xs)]
        torch.cuda.synchronize()
        return outs

    monkeypatch.setattr(L, "PREFETCH_NEXT", False)
    ref = steps(2)
    monkeypatch.setattr(L, "PREFETCH_NEXT", True)
    hints = []
    lib = _lib.load()
    real = lib.sdnq_hip_prefetch_hint

    def spy(*a):
        hints.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "sdnq_hip_prefetch_hint", spy, raising=False)
    L._prefetch_chain.reset()
    n0 = L._FP.last_hint()[0] if L._FP is not None else 0
    got = steps(3)
    if L._FP is not None:  # the chain lives in the fast-path module (csrc/fastpath.cpp), which calls the library itself
        last = L._FP.last_hint()
        assert last[0] - n0 >= 2 * (len(mods) - 1) and last[1] and last[2]
    else:
        assert len(hints) >= 2 * (len(mods) - 1) and any(h[2] for h in hints)  # steps 2 and 3 name the next unit(s)
    for a, b in zip(ref, got):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    w = L._state(mods[0]).mm_weight
    _lib.check(lib.sdnq_hip_prefetch(w.data_ptr(), w.numel(), 0, torch.cuda.current_stream().cuda_stream), "prefetch")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_load_sdnq_model_computes_what_the_reference_computed(gpu_device):
    """The checkpoint the reference wrote and re-loaded (tests/golden/make_golden_checkpoint.py), loaded here WITHOUT the reference:
    every quantized layer, fed the input the reference's layer saw, returns the reference's output -- bit for bit for the int8
    direct-matmul and the uint4 -> int8 re-quantized layer, within one bf16 ulp for the int8 + SVD layer (the addmm's summation
    order) -- and the whole model agrees end to end."""
    import os
    import sdnq_amd
    from tests.test_host_logic import TinyNet
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoint_tiny")
    model = sdnq_amd.load_sdnq_model(path, model_cls=TinyNet, device=gpu_device)
    io = np.load(os.path.join(path, "io.npz"))
    bf = lambda a: torch.from_numpy(a.astype(np.int32).astype(np.int16)).view(torch.bfloat16).to(gpu_device)  # noqa: E731
    for name, exact in (("proj_in", True), ("mid", True), ("proj_out", False)):
        got = getattr(model, name)(bf(io[f"{name}.in"]))
        want = bf(io[f"{name}.out"])
        if exact:
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name
        else:
            ulp = want.float().abs().clamp_min(2.0 ** -126) * 2.0 ** -7
            assert bool(((got.float() - want.float()).abs() <= ulp).all()), name
    with torch.no_grad():
        y = model(bf(io["x"])).float()
    want = bf(io["y"]).float()
    assert float((y - want).abs().max()) <= 0.05 * float(want.abs().max())
