"""Pins the CPU oracle (oracle/) against vectors captured from the imported reference.

Bit-exact where the arithmetic is order-free (unpack, dequant, activation quantization, int8 matmul);
stated tolerances where the reference's own GEMM summation order is unspecified.
"""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.golden_util import GOLD, Case, case_names


def ulp_bf16(ref):
    return np.maximum(np.abs(ref), 1e-30) * 2.0 ** -7


def test_dtype_table_matches_reference():
    table = json.load(open(os.path.join(GOLD, "dtype_table.json")))
    for name, ent in table.items():
        if name in ("float32", "fp32", "int32", "uint32", "float8_e8m0fnu", "float8_e4m3fnuz", "float8_e5m2fnuz"):
            continue
        info = O.dtype_info(name)
        assert info["bits"] == ent["num_bits"], name
        assert info["packed"] == ent["is_packed"] or (not ent["is_integer"] and ent["num_bits"] in (8, 16)), name
        if not ent["is_integer"]:
            assert (info["exponent"], info["mantissa"]) == (ent["exponent"], ent["mantissa"]), name
            assert (info["kind"] == "ufloat") == ent["is_unsigned"], name
        else:
            assert (info["kind"] == "uint") == ent["is_unsigned"], name


def test_int_codecs_known_answers():
    z = np.load(os.path.join(GOLD, "codecs.npz"))
    for bits in list(range(1, 8)) + list(range(9, 16)):
        vals = z[f"uint{bits}.values"]
        packed = z[f"uint{bits}.packed"]
        got = O.unpack_codes(packed, bits, vals.size)
        assert np.array_equal(got, vals), f"unpack uint{bits}"
        mine = O.pack_codes(vals, bits)
        ref = packed.reshape(-1)
        if ref.dtype == np.int64:  # 1-bit: the reference's bool packing promotes to int64 words holding 8 bits each
            ref = ref.astype(np.uint8)
        ref = ref.view(np.uint8) if bits < 8 else ref.view(np.uint16)
        assert np.array_equal(mine, ref), f"pack uint{bits}"


def test_float_decode_tables():
    z = np.load(os.path.join(GOLD, "codecs.npz"))
    meta = json.load(open(os.path.join(GOLD, "codecs.json")))
    n = 0
    for name, ent in meta.items():
        if not name.startswith("float"):
            continue
        codes, dec = z[f"{name}.codes"], z[f"{name}.decoded"]
        L = O.lib()
        mine = np.array([L.orc_decode_exmy(int(c), ent["exponent"], ent["mantissa"], int(ent["is_unsigned"])) for c in codes],
                        dtype=np.float32)
        assert np.array_equal(mine.view(np.uint32), dec.view(np.uint32)), name  # bit patterns: -0.0 codes decode to +0.0
        # decode of the reference-packed sweep
        info = O.dtype_info(name)
        got = O.weight_values(z[f"{name}.sweep_packed"], name, (480,))
        assert np.array_equal(got, z[f"{name}.sweep_decoded"]), name
        n += 1
    assert n >= 55


def test_hadamard_matrices_and_scales():
    z = np.load(os.path.join(GOLD, "hadamard.npz"))
    for n in (4, 8, 16, 32, 64, 128, 256, 512):
        assert np.array_equal(O.hadamard_matrix(n, "f32"), z[f"H{n}"]), n


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_hadamard_rotation(dt):
    z = np.load(os.path.join(GOLD, "hadamard.npz"))
    for n in (64, 128, 256):
        x = O.from_bits(z[f"x_{dt}_{n}"], dt)
        y = O.from_bits(z[f"y_{dt}_{n}"], dt)
        got = O.rotate_hadamard(x, n, dt)
        # summation order of the reference GEMM is unspecified: allow 1 ulp of the dtype on a few elements
        tol = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10, "f32": 2.0 ** -18}[dt]
        assert np.all(np.abs(got - y) <= tol * np.maximum(np.abs(y), np.abs(y).max() if dt == "f32" else 1.0)), (dt, n)
        assert np.mean(got != y) < (0.01 if dt != "f32" else 1.0), (dt, n)


def test_dequant_all_storage_dtypes_bit_exact():
    z = np.load(os.path.join(GOLD, "dequant_dtypes.npz"))
    meta = json.load(open(os.path.join(GOLD, "dequant_dtypes.json")))["dtypes"]
    assert len(meta) >= 80
    for key, ent in meta.items():
        deq = ent["deq"]
        zp = z[f"{key}.zero_point"] if ent["tensors"]["zero_point"]["dtype"] != "none" else None
        mod = O.OracleLinear(deq, z[f"{key}.weight"], z[f"{key}.scale"], zp, N=16, K=128)
        got = mod.dequantize("f32")
        assert np.array_equal(got, z[f"{key}.out"].reshape(16, 128)), key


@pytest.mark.parametrize("name", case_names())
def test_case_dequant_and_requant(name):
    c = Case(name)
    mod = c.oracle_module()
    ref32 = c.f32("w_dequant_f32_nohad").reshape(c.N, c.K)
    got32 = mod.dequantize("f32", hadamard=False)
    if c.has("svd_up"):
        tol = ulp_bf16(ref32) if c.tag != "f16" else np.maximum(ulp_bf16(ref32), 2.0 ** -24)  # f16 addmm: one subnormal step near 0
        tol = np.maximum(tol, 1e-8)  # results that cancel to ~0: the ulp of the RESULT says nothing about the addends' rounding
        assert np.all(np.abs(got32 - ref32) <= tol), name  # addmm in bf16: <= 1 bf16 ulp
        assert np.mean(got32 != ref32) < 1e-3
    else:
        assert np.array_equal(got32, ref32), name
    ref = c.f32("w_dequant").reshape(c.N, c.K)
    got = mod.dequantize(c.tag)
    if c.deq["use_hadamard"] or c.has("svd_up"):
        assert np.all(np.abs(got - ref) <= 2 * ulp_bf16(ref) + 1e-6), name
    else:
        assert np.array_equal(got, ref), name
    if c.has("requant_weight"):
        wq, ws, *wzp = mod.re_quantize_matmul()
        rw = c.raw("requant_weight").reshape(c.K, c.N).T  # logical [K,N] -> [N,K]
        assert np.array_equal(ws, c.f32("requant_scale").reshape(-1)), name
        assert len(wzp) == int(c.has("requant_zero_point"))
        if wzp:  # re_quantize_uint_mm (dequantizer.py:178-187)
            assert np.array_equal(wzp[0], c.f32("requant_zero_point").reshape(-1)), name  # (values: bf16 bits under 16-bit scales)
        if wq.dtype == np.float16:  # the float16 matmul's operand (fixtures hold 16-bit floats as their bit patterns)
            assert np.array_equal(wq.view(np.uint16), rw.view(np.uint16)), name
        else:
            assert np.array_equal(wq.view(np.uint8), rw.view(np.uint8)), name


@pytest.mark.parametrize("name", case_names())
def test_case_forward(name):
    c = Case(name)
    mod = c.oracle_module()
    d = c.deq
    for M in c.ms():
        x = c.f32(f"x_{M}")
        y_ref = c.f32(f"y_{M}")
        y, inter = O.forward(mod, x, c.tag, want_intermediates=True)
        assert y.shape == y_ref.shape
        qmm = d["use_quantized_matmul"] and M >= 32
        exact_int = (qmm and d["quantized_matmul_dtype"] in ("int8", "uint8") and not d["use_hadamard"] and not c.has("svd_up"))
        if qmm and c.has(f"xq_{M}") and not d["use_hadamard"]:
            assert np.array_equal(inter["xq"].view(np.uint8), c.raw(f"xq_{M}").view(np.uint8)), (name, M)
            assert np.array_equal(inter["xs"], c.f32(f"xs_{M}").reshape(-1)), (name, M)
        if exact_int:
            assert np.array_equal(y, y_ref), (name, M)  # int32 accumulate is exact; fma epilogue
        else:
            scale = np.abs(y_ref).max()
            err = np.abs(y - y_ref).max() / scale
            # fp8 / Hadamard / SVD / bf16-linear: accumulation-order noise then one bf16/f16 rounding
            assert err <= (2e-2 if d["use_hadamard"] else 8e-3), (name, M, err)
            rel_l2 = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
            assert rel_l2 <= (2e-3 if c.tag != "f32" else 1e-5), (name, M, rel_l2)


# ---- conv ---------------------------------------------------------------------
from tests.golden_util import ConvCase, conv_case_names  # noqa: E402


@pytest.mark.parametrize("name", conv_case_names())
def test_conv_case_dequant_and_forward(name):
    """Oracle conv = im2col + the Linear arithmetic with per-kernel-position scales, against the reference's conv forwards."""
    c = ConvCase(name)
    d = c.deq
    omod = c.oracle_module()
    if c.has("w_dequant"):
        W = omod.dequantize(c.tensor_tag("w_dequant"), use_svd=True)
        ref = c.f32("w_dequant").reshape(c.N, c.K)
        if c.has("svd_up"):
            assert np.abs(W - ref).max() <= 2.0 ** -8 * np.abs(ref).max()
        elif d["use_hadamard"] and c.tag == "f32":  # the un-rotation is an fp32 matmul: summation order is the library's
            assert np.abs(W - ref).max() <= 1e-6 * np.abs(ref).max(), (name, "dequant")
        elif d["use_hadamard"]:  # ... and in a 16-bit dtype that order flips the last bit of a few elements (the Linear cases' bound)
            assert np.all(np.abs(W - ref) <= 2 * ulp_bf16(ref) + 1e-6) and np.mean(W != ref) < 1e-3, (name, "dequant")
        else:
            assert np.array_equal(W, ref), (name, "dequant")
    if c.has("requant_weight"):
        wq, ws = omod.re_quantize_matmul()[:2]
        rw = c.raw("requant_weight")  # logical [K, N]
        assert np.array_equal(wq.view(np.uint8), np.ascontiguousarray(rw.T).view(np.uint8)), (name, "requant codes")
        assert np.array_equal(ws, c.f32("requant_scale").reshape(-1)), (name, "requant scale")
    for i in c.inputs():
        x = c.f32(f"x_{i}")
        y = O.conv_forward(omod, x, c.conv, c.tag)
        ref = c.f32(f"y_{i}")
        assert y.shape == ref.shape
        # int8 accumulation is exact and the epilogue's roundings are the reference's, term by term -- for the uint8 (asymmetric) matmul too:
        # its K * xzp * wzp term is built in the conv forwards' own order (conv_uint8.py:66), round 4
        exact = d["use_quantized_matmul"] and d["quantized_matmul_dtype"] in ("int8", "uint8") and not c.has("svd_up") and not d["use_hadamard"]
        if exact:
            assert np.array_equal(y, ref), (name, i, int((y != ref).sum()))
        else:
            scale = float(np.abs(ref).max())
            lim = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10, "f32": 2e-6}[c.tag]
            assert np.abs(y - ref).max() <= lim * scale, (name, i, float(np.abs(y - ref).max()), scale)


# Where the fixtures come from is checked by the scripts that made them, run by hand on a host where the reference is installed
# (they execute the reference's own code, which is not part of this repository): tests/golden/make_golden.py --verify,
# make_golden_checkpoint.py [--verify DIR], make_golden_hf.py DIR, and the random sweeps tools/fuzz_oracle_vs_reference.py and
# tools/fuzz_quantizer_vs_reference.py.  The tests above pin the oracle to the stored fixtures alone.
