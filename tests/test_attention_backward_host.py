"""Quantized attention backward, host side: the CPU restatement (tests/attn_bwd_util.py) against the reference kernels' fixtures
(tests/golden/abwd_*), the public signature, the options outside the built scope and the import-name drop-in."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests import attn_bwd_util as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def abwd_names(dtype=None):
    names = sorted(f[5:-5] for f in os.listdir(GOLD) if f.startswith("abwd_") and f.endswith(".json"))
    return [n for n in names if dtype is None or n.startswith(dtype + "_")]


def load(name):
    meta = json.load(open(os.path.join(GOLD, f"abwd_{name}.json")))
    z = np.load(os.path.join(GOLD, f"abwd_{name}.npz"))
    view = {"f16": torch.float16, "bf16": torch.bfloat16, "bool": torch.bool}
    out = {}
    for key, info in meta["tensors"].items():
        t = torch.from_numpy(np.ascontiguousarray(z[key]))
        if info["dtype"] in view:
            t = t.view(view[info["dtype"]])
        out[key] = t.reshape(info["shape"])
    return meta, out


def prepared_mask(mask, qn, kn):
    if mask is None:
        return None
    m = mask.to(torch.int8) if mask.dtype == torch.bool else mask
    while m.ndim < 4:
        m = m.unsqueeze(0)
    return m.expand(-1, -1, qn, kn) if m.shape[-2] == 1 else m


def restate(meta, t):
    kw = meta["kwargs"]
    sh = meta["shape"]
    d = sh["d"]
    sm_scale = kw.get("scale") or d ** -0.5
    return R.backward(t["q_q"], t["q_scale"], t["k_q"], t["k_scale"], t["v"], t["do"], t["out"], t["lse"], sm_scale,
                      is_causal=kw.get("is_causal", False), mask=prepared_mask(t.get("mask"), sh["qn"], sh["kn"]),
                      hadamard_group=meta["hadamard_group"])


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@pytest.mark.parametrize("name", abwd_names("f16"))
def test_restatement_reproduces_reference_backward(name):
    meta, t = load(name)
    dq, dk, dv = restate(meta, t)
    for key, mine in (("dq", dq), ("dk", dk), ("dv", dv)):
        ref = t[key]
        assert mine.shape == ref.shape
        assert rel(mine, ref) < 2e-3, (key, rel(mine, ref))
        # and it is far closer to the reference kernel than the reference is to exact fp32 attention
        assert rel(mine, ref) < 0.1 * rel(ref, t["exact_" + key]), key


def test_fixtures_cover_the_issue_range():
    names = abwd_names()
    assert len(names) >= 13
    metas = [load(n)[0] for n in names]
    assert any(m["shape"]["kn"] % 32 and m["kwargs"].get("is_causal") for m in metas)          # causal with a key tail
    assert any(m["shape"]["qh"] != m["shape"]["kh"] and m["shape"]["d"] == 128 for m in metas)  # grouped heads at d128
    assert {40, 80} <= {m["shape"]["d"] for m in metas}
    assert {64, 32} <= {m["hadamard_group"] for m in metas}
    assert all(m["block_m"] == 32 and m["block_n"] == 32 for m in metas)
    assert any(m["dtype"] == "bf16" and "grads_are" in m for m in metas)


def test_signature_matches_reference():
    from sdnq_amd.attention import sdnq_hip_atten_with_backward
    params = inspect.signature(sdnq_hip_atten_with_backward).parameters
    expected = [("query", inspect.Parameter.empty), ("key", inspect.Parameter.empty), ("value", inspect.Parameter.empty), ("attn_mask", None),
                ("dropout_p", 0.0), ("is_causal", False), ("scale", None), ("enable_gqa", False), ("smooth_k", True), ("use_hadamard", False),
                ("hadamard_group_size", 256), ("matmul_dtype", "int8"), ("pv_matmul_dtype", None), ("do_quantize", True),
                ("use_fp16_accum", False), ("out_dtype", None)]
    assert [(n, p.default) for n, p in params.items()] == expected


@pytest.mark.parametrize("kw, words", [
    (dict(matmul_dtype="fp8"), "matmul_dtype"),
    (dict(matmul_dtype="float8_e4m3fn"), "matmul_dtype"),
    (dict(pv_matmul_dtype="int8"), "pv_matmul_dtype"),
    (dict(pv_matmul_dtype="float16"), "pv_matmul_dtype"),
    (dict(use_fp16_accum=True), "use_fp16_accum"),
    (dict(do_quantize=False), "do_quantize"),
])
def test_unbuilt_options_raise(kw, words):
    from sdnq_amd.attention import sdnq_hip_atten_with_backward
    q = torch.zeros(1, 2, 32, 64, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match=words):
        sdnq_hip_atten_with_backward(q, q, q, **kw)


def test_cpu_tensors_raise():
    from sdnq_amd import _lib
    from sdnq_amd.attention import sdnq_hip_atten_with_backward
    q = torch.zeros(1, 2, 32, 64, dtype=torch.float16, requires_grad=True)
    with pytest.raises(_lib.SdnqHipError):
        sdnq_hip_atten_with_backward(q, q, q)


def test_import_name_drop_in():
    from sdnq.kernels.triton_atten import sdnq_triton_atten
    from sdnq.kernels.triton_atten_backward import sdnq_triton_atten_with_backward
    from sdnq_amd.attention import sdnq_hip_atten, sdnq_hip_atten_with_backward
    assert sdnq_triton_atten is sdnq_hip_atten
    assert sdnq_triton_atten_with_backward is sdnq_hip_atten_with_backward
