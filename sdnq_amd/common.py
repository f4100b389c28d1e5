"""Storage-dtype table and layer-type constants of the SDNQ format.

Mirrors the *contents* of the reference's ``dtype_dict`` (src/sdnq/common.py:16-267) -- 212 rows:
per-dtype ``min/max/num_bits/sign/exponent/mantissa/target_dtype/torch_dtype/storage_dtype/
is_unsigned/is_integer/is_packed`` -- but builds them from the format rules instead of a literal:

* ``intN`` / ``uintN`` (N = 1..16, 32): two's-complement range; sub-byte and 9..15-bit types are
  packed (``is_packed``) into uint8 / int16 words.
* ``float{B}_e{E}m{M}fn`` (signed) and ``...fnu`` (unsigned): every exponent code is finite, bias
  2^(E-1)-1, so max = 2^(2^E-1-bias) * (2 - 2^-M); codes are packed unless B is 8 or 16.
* native torch types (float32/bfloat16/float16/float8_e4m3fn/float8_e5m2/...) are not packed.

``tests/test_common.py`` checks this table against the fixture captured from the reference.
"""
from __future__ import annotations

import torch

sdnq_version = "0.2.5"
sdnq_keys = {"weight", "scale", "zero_point", "svd_up", "svd_down"}  # reference common.py:8


def _int_entry(bits: int, unsigned: bool) -> dict:
    if bits in (8, 16, 32):
        tdt = getattr(torch, ("uint" if unsigned else "int") + str(bits))
        target, storage, packed = tdt, tdt, False
    elif bits == 1:
        tdt, target, storage, packed = torch.bool, torch.bool, torch.bool, True
    else:
        name = ("uint" if unsigned else "int") + str(bits)
        if bits < 8:
            tdt = torch.uint8 if unsigned else torch.int8
            storage = torch.uint8
        else:
            tdt, storage = torch.int16, torch.int16
        target, packed = name, True
    if unsigned:
        # the reference lists 2^N (not 2^N - 1) as the max of the 9..15-bit unsigned containers
        mx = (1 << bits) if 9 <= bits <= 15 else (1 << bits) - 1
        return {"min": 0, "max": mx, "num_bits": bits, "sign": 0, "exponent": 0, "mantissa": bits,
                "target_dtype": target, "torch_dtype": tdt, "storage_dtype": storage,
                "is_unsigned": True, "is_integer": True, "is_packed": packed}
    return {"min": -(1 << (bits - 1)), "max": (1 << (bits - 1)) - 1, "num_bits": bits, "sign": 1, "exponent": 0,
            "mantissa": bits - 1, "target_dtype": target, "torch_dtype": tdt, "storage_dtype": storage,
            "is_unsigned": False, "is_integer": True, "is_packed": packed}


def _custom_float_entry(bits: int, e: int, m: int, unsigned: bool) -> dict:
    bias = (1 << (e - 1)) - 1
    mx = float(2.0 ** ((1 << e) - 1 - bias) * (2.0 - 2.0 ** (-m)))
    storage = torch.uint8 if bits <= 8 else (torch.uint16 if bits == 16 else torch.int16)
    return {"min": 0 if unsigned else -mx, "max": mx, "num_bits": bits, "sign": 0 if unsigned else 1, "exponent": e,
            "mantissa": m, "target_dtype": f"fp{bits}", "torch_dtype": torch.float32, "storage_dtype": storage,
            "is_unsigned": unsigned, "is_integer": False, "is_packed": True}


def _native_float_entry(tdt: torch.dtype, bits: int, e: int, m: int, mx: float, target=None) -> dict:
    return {"min": -mx, "max": mx, "num_bits": bits, "sign": 1, "exponent": e, "mantissa": m,
            "target_dtype": tdt if target is None else target, "torch_dtype": tdt, "storage_dtype": tdt,
            "is_unsigned": False, "is_integer": False, "is_packed": False}


def _build_dtype_dict() -> dict:
    d = {}
    for bits in (32, 16, 8, 15, 14, 13, 12, 11, 10, 9, 7, 6, 5, 4, 3, 2):
        d[f"int{bits}"] = _int_entry(bits, False)
    for bits in (32, 16, 8, 15, 14, 13, 12, 11, 10, 9, 7, 6, 5, 4, 3, 2, 1):
        d[f"uint{bits}"] = _int_entry(bits, True)
    d["float32"] = _native_float_entry(torch.float32, 32, 8, 23, 3.40282e+38)
    d["bfloat16"] = _native_float_entry(torch.bfloat16, 16, 8, 7, 3.38953e+38)
    d["float16"] = _native_float_entry(torch.float16, 16, 5, 10, 65504.0)
    d["float8_e4m3fn"] = _native_float_entry(torch.float8_e4m3fn, 8, 4, 3, 448.0)
    d["float8_e5m2"] = _native_float_entry(torch.float8_e5m2, 8, 5, 2, 57344.0)
    for bits in range(16, 0, -1):
        for e in range(1, 6):
            m = bits - 1 - e
            if m >= 0 and bits >= 2:
                name = f"float{bits}_e{e}m{m}fn"
                if name == "float8_e4m3fn":  # the native OCP type owns that name; the custom codec is "_sdnq"
                    name = "float8_e4m3fn_sdnq"
                d[name] = _custom_float_entry(bits, e, m, False)
            m = bits - e
            if m >= 0:
                d[f"float{bits}_e{e}m{m}fnu"] = _custom_float_entry(bits, e, m, True)
    return d


dtype_dict = _build_dtype_dict()

# aliases (reference common.py:230-267)
dtype_dict["fp32"] = dtype_dict["float32"]
dtype_dict["bf16"] = dtype_dict["bfloat16"]
dtype_dict["fp16"] = dtype_dict["float16"]
dtype_dict["fp8"] = dtype_dict["float8_e4m3fn"]
_DEFAULT_E = {1: 1, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 3, 8: 4, 9: 4}
for _b in range(1, 17):
    _e = _DEFAULT_E.get(_b, 5)
    if _b >= 2 and _b not in (8, 16):
        dtype_dict[f"fp{_b}"] = dtype_dict[f"float{_b}_e{_e}m{_b - 1 - _e}fn"]
    dtype_dict[f"ufp{_b}"] = dtype_dict[f"float{_b}_e{_e}m{_b - _e}fnu"]
dtype_dict["fp1"] = dtype_dict["float1_e1m0fnu"]
dtype_dict["int1"] = dtype_dict["uint1"]
dtype_dict["bool"] = dtype_dict["uint1"]

if hasattr(torch, "float8_e8m0fnu"):
    dtype_dict["float8_e8m0fnu"] = {"min": -1.70141e+38, "max": 1.70141e+38, "num_bits": 8, "sign": 1, "exponent": 8,
                                    "mantissa": 0, "target_dtype": "fp8", "torch_dtype": torch.float8_e8m0fnu,
                                    "storage_dtype": torch.float8_e8m0fnu, "is_unsigned": False, "is_integer": False,
                                    "is_packed": False}
if hasattr(torch, "float8_e4m3fnuz"):
    dtype_dict["float8_e4m3fnuz"] = {"min": -240.0, "max": 240.0, "num_bits": 8, "sign": 1, "exponent": 4, "mantissa": 3,
                                     "target_dtype": "fp8", "torch_dtype": torch.float8_e4m3fnuz,
                                     "storage_dtype": torch.float8_e4m3fnuz, "is_unsigned": False, "is_integer": False,
                                     "is_packed": False}
if hasattr(torch, "float8_e5m2fnuz"):
    dtype_dict["float8_e5m2fnuz"] = {"min": -57344.0, "max": 57344.0, "num_bits": 8, "sign": 1, "exponent": 5,
                                     "mantissa": 2, "target_dtype": "fp8", "torch_dtype": torch.float8_e5m2fnuz,
                                     "storage_dtype": torch.float8_e5m2fnuz, "is_unsigned": False, "is_integer": False,
                                     "is_packed": False}

torch_dtype_dict = {
    torch.int32: "int32", torch.int16: "int16", torch.int8: "int8", torch.uint32: "uint32", torch.uint16: "uint16",
    torch.uint8: "uint8", torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16",
    torch.float8_e4m3fn: "float8_e4m3fn", torch.float8_e5m2: "float8_e5m2",
}


def _build_weights_dtype_order() -> list:
    """Candidate order of the dynamic dtype search (the reference's weights_dtype_order, common.py:302-334), by its rule: for every
    width B = 1..16 the signed formats -- intB, the native OCP floats of that width, the custom eXmYfn floats by ascending exponent
    (E <= 5) -- then the unsigned ones -- uintB, the eXmYfnu floats by ascending exponent.  (There is no int1 / signed 1-bit float.)"""
    order = []
    for bits in range(1, 17):
        if bits >= 2:
            order.append(f"int{bits}")
            order += {8: ["float8_e4m3fn", "float8_e5m2"], 16: ["float16"]}.get(bits, [])
            for e in range(1, min(5, bits - 1) + 1):
                name = f"float{bits}_e{e}m{bits - 1 - e}fn"
                order.append("float8_e4m3fn_sdnq" if name == "float8_e4m3fn" else name)
        order.append(f"uint{bits}")
        order += [f"float{bits}_e{e}m{bits - e}fnu" for e in range(1, min(5, bits) + 1)]
    return order


weights_dtype_order = _build_weights_dtype_order()

linear_types = {"Linear", "SDNQLinear"}
embedding_types = {"Embedding", "SDNQEmbedding", "Gemma4TextScaledWordEmbedding"}
conv_types = {"Conv1d", "Conv2d", "Conv3d", "SDNQConv1d", "SDNQConv2d", "SDNQConv3d"}
conv_transpose_types = {"ConvTranspose1d", "ConvTranspose2d", "ConvTranspose3d", "SDNQConvTranspose1d",
                        "SDNQConvTranspose2d", "SDNQConvTranspose3d"}
allowed_types = set.union(linear_types, embedding_types, conv_types, conv_transpose_types)

accepted_weight_dtypes = set(dtype_dict.keys())
accepted_matmul_dtypes = {"int8", "uint8", "fp8", "fp16", "float8_e4m3fn", "float16"}


def compile_func(fn, **kwargs):  # the reference wraps hot functions in torch.compile (common.py:356); here the
    return fn                     # hot path is hand-written HIP, so this is the identity.
