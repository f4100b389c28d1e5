#!/usr/bin/env python3
"""Capture golden vectors of DYNAMIC quantization (use_dynamic_quantization=True) from the REAL reference (Disty0/sdnq @ /root/reference).

Runs ONLY in the build container, like make_golden.py (same environment switches, same stand-in ``diffusers``, whose helpers it
imports): the reference's ``apply_sdnq_to_module`` quantizes a small model of float Linear / conv / embedding layers with
``use_dynamic_quantization=True`` on CPU, and ``dyn_<case>.npz / .json`` receive, per layer, the float weight, the stored tensors and
the dequantizer record (or "float" when no candidate passed), the config lists after the call, and EVERY candidate the search
evaluated with its mse_loss -- captured by wrapping ``torch.nn.functional.mse_loss`` while the reference runs.  The fixtures are DATA
only: no reference source is stored.

A case is refused when a candidate's loss / var(W) lies within 1e-3 (relative) of its threshold -- 2x for SVD cases, whose factors
come from a random solver -- so that the choice does not hinge on the last bits of a float sum.

Usage:  python tests/golden/make_golden_dynamic.py [<case name> ...]
        python tests/golden/make_golden_dynamic.py --verify        # re-run the reference: same choices, lists, losses and tensors
        python tests/golden/make_golden_dynamic.py --regen-check   # regenerate into a temp dir, compare with the tracked files

Every case is self-seeded (`torch.manual_seed(crc32(name))` before quantizing: the SVD case draws from the global generator).
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (environment switches, stand-in diffusers, the reference on sys.path, to_np / from_np / deq_fields)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdnq.quantizer as RQ  # noqa: E402  (the reference)
from sdnq import SDNQConfig  # noqa: E402

OUT_DIR = HERE  # --regen-check points this at a temp dir

# layers: (name, kind, shape args, scale of the random weight); kind linear (K, N), conv (cin, cout, k), embedding (V, D)
CASES = [
    dict(name="lin_first_int8", dtype="bf16", layers=[("proj", "linear", (256, 64), 0.02)], cfg=dict(weights_dtype="int8")),
    dict(name="lin_walk_int2", dtype="f32", layers=[("proj", "linear", (256, 64), 0.02)],
         cfg=dict(weights_dtype="int2", dynamic_loss_threshold=2e-3)),
    dict(name="lin_exhaust_float", dtype="f16", layers=[("proj", "linear", (64, 32), 0.02)],
         cfg=dict(weights_dtype="uint14", dynamic_loss_threshold=0.0, minimum_allowed_numel=1024)),
    dict(name="lin_int8_qmm_past8", dtype="bf16", layers=[("proj", "linear", (256, 64), 0.02)],
         cfg=dict(weights_dtype="int8", dynamic_loss_threshold=1e-6, use_quantized_matmul=True)),
    dict(name="lin_had_uint4", dtype="bf16", layers=[("proj", "linear", (512, 64), 0.02)],
         cfg=dict(weights_dtype="uint4", use_hadamard=True, hadamard_group_size=128, dynamic_loss_threshold=2e-3)),
    dict(name="lin_svd_int4", dtype="bf16", layers=[("proj", "linear", (512, 64), 0.02)],
         cfg=dict(weights_dtype="int4", use_svd=True, svd_rank=8, use_quantized_matmul=True, dynamic_loss_threshold=2e-3)),
    dict(name="lin_codebook_uint2", dtype="f32", layers=[("proj", "linear", (256, 64), 0.02)],
         cfg=dict(weights_dtype="uint2", use_codebook=True, dynamic_loss_threshold=1e-3)),
    dict(name="conv_uint4", dtype="f16", layers=[("conv", "conv", (32, 64, 3), 0.05)],
         cfg=dict(weights_dtype="uint4", quant_conv=True, dynamic_loss_threshold=2e-3)),
    dict(name="emb_int4", dtype="bf16", layers=[("embed", "embedding", (128, 256), 0.02)],
         cfg=dict(weights_dtype="int4", quant_embedding=True, dynamic_loss_threshold=2e-3)),
    dict(name="model_module_threshold", dtype="bf16", layers=[("q", "linear", (256, 64), 0.02), ("k", "linear", (256, 64), 0.02)],
         cfg=dict(weights_dtype="int4", modules_quant_config={"k": {"dynamic_loss_threshold": 1e-4}})),
    dict(name="model_mixed", dtype="bf16",
         layers=[("a", "linear", (256, 64), 0.02), ("b", "linear", (256, 64), "heavy"), ("c", "linear", (512, 64), "outlier"),
                 ("d", "linear", (64, 256), 0.02)],
         cfg=dict(weights_dtype="uint3", dynamic_loss_threshold=3e-3, use_quantized_matmul=True)),
]


def _weight(case, lname, kind, shape, scale):
    g = torch.Generator().manual_seed(zlib.crc32(f"{case['name']}.{lname}".encode()))
    if kind == "linear":
        k, n = shape
        full = (n, k)
    elif kind == "conv":
        cin, cout, ks = shape
        full = (cout, cin, ks, ks)
    else:
        full = shape
    w = torch.randn(full, generator=g)
    if scale == "heavy":  # heavy tails: a Student-t-like weight needs more bits
        w = w / (torch.rand(full, generator=g) + 0.05) * 0.002
    elif scale == "outlier":  # a few strong input channels
        w = w * 0.02
        w[:, torch.randperm(full[1], generator=g)[:4]] *= 20.0
    else:
        w = w * scale
    return w


def make_model(case):
    dtype = G.TORCH_DT[case["dtype"]]
    model = torch.nn.Module()
    for lname, kind, shape, scale in case["layers"]:
        if kind == "linear":
            layer = torch.nn.Linear(shape[0], shape[1], bias=False)
        elif kind == "conv":
            layer = torch.nn.Conv2d(shape[0], shape[1], shape[2], padding=1, bias=False)
        else:
            layer = torch.nn.Embedding(*shape)
        with torch.no_grad():
            layer.weight.copy_(_weight(case, lname, kind, shape, scale))
        setattr(model, lname, layer.to(dtype))
    return model


def config(case):
    cfg = dict(case["cfg"])
    cfg.setdefault("minimum_allowed_numel", 4096)
    return SDNQConfig(use_dynamic_quantization=True, **cfg)


def quantize(case):
    """-> (quantized model, config after the call, candidates [(param, dtype, mse)])"""
    torch.manual_seed(zlib.crc32(case["name"].encode()))
    model = make_model(case)
    cfg = config(case)
    trace, current = [], {}
    real_mse, real_qlw = torch.nn.functional.mse_loss, RQ.sdnq_quantize_layer_weight

    def qlw(weight, *a, **kw):
        current["dtype"], current["param"] = kw["weights_dtype"], kw.get("param_name")
        return real_qlw(weight, *a, **kw)

    def mse(a, b, *args, **kw):
        out = real_mse(a, b, *args, **kw)
        trace.append((current["param"], current["dtype"], float(out)))
        return out

    RQ.sdnq_quantize_layer_weight, torch.nn.functional.mse_loss = qlw, mse
    try:
        with torch.no_grad():
            model, cfg = RQ.apply_sdnq_to_module(model, cfg)
    finally:
        RQ.sdnq_quantize_layer_weight, torch.nn.functional.mse_loss = real_qlw, real_mse
    return model, cfg, trace


def _threshold(case, lname):
    cfg = dict(case["cfg"])
    cfg.update(cfg.get("modules_quant_config", {}).get(lname, {}))
    t = cfg.get("dynamic_loss_threshold")
    if t is None or t < 0:
        t = 10 ** -(_bits(cfg["weights_dtype"]) / 2)
    return t


def _bits(name):
    from sdnq.common import dtype_dict
    return dtype_dict[name]["num_bits"]


def run_case(case, check_margin=True):
    name = case["name"]
    floats = make_model(case)
    model, cfg, trace = quantize(case)
    arrays, tensors, layers = {}, {}, {}

    def put(key, t):
        a, tag = G.to_np(t)
        tensors[key] = {"shape": None if t is None else list(t.shape), "stride": None if t is None else list(t.stride()), "dtype": tag}
        if a is not None:
            arrays[key] = a

    margin = 2e-3 if case["cfg"].get("use_svd") else 1e-3
    for lname, kind, _shape, _scale in case["layers"]:
        pname = lname + ".weight"
        w = getattr(floats, lname).weight.detach()
        put(f"{lname}.w_float", w)
        var = float(w.to(torch.float32).std().square().clamp(min=1e-8))
        thr = _threshold(case, lname)
        layer = getattr(model, lname)
        dq = getattr(layer, "sdnq_dequantizer", None)
        for k in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
            put(f"{lname}.{k}", getattr(layer, k, None) if dq is not None else None)
        cands = [(d, m) for p, d, m in trace if p == pname]
        for d, m in cands:
            loss = float(np.float32(m) / np.float32(var))
            if check_margin and abs(loss - thr) <= margin * max(thr, 1e-30):
                raise SystemExit(f"{name}/{lname}: candidate {d} loss {loss:.6e} lies within {margin} of the threshold {thr:.6e}")
        layers[lname] = dict(param=pname, kind=kind, chosen=dq.weights_dtype if dq is not None else "float",
                             deq=G.deq_fields(dq) if dq is not None else None, var=var, threshold=thr,
                             candidates=[d for d, _ in cands], mse=[m for _, m in cands])
    lists = dict(modules_dtype_dict=cfg.modules_dtype_dict, modules_to_not_use_matmul=cfg.modules_to_not_use_matmul,
                 modules_to_not_convert=cfg.modules_to_not_convert)
    meta = dict(name=name, dtype=case["dtype"], cfg=case["cfg"], layers=layers, lists=lists, tensors=tensors,
                geometry={lname: [kind, list(shape)] for lname, kind, shape, _ in case["layers"]})
    np.savez_compressed(os.path.join(OUT_DIR, f"dyn_{name}.npz"), **arrays)
    with open(os.path.join(OUT_DIR, f"dyn_{name}.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", name, {k: (v["chosen"], len(v["candidates"])) for k, v in layers.items()})
    return meta, arrays


def verify():
    """Re-run the reference on each case: the same choices, lists and candidate losses, and the same stored tensors bit for bit."""
    bad = 0
    for case in CASES:
        name = case["name"]
        z = np.load(os.path.join(HERE, f"dyn_{name}.npz"))
        with open(os.path.join(HERE, f"dyn_{name}.json")) as f:
            meta = json.load(f)
        model, cfg, trace = quantize(case)
        ok = json.loads(json.dumps(dict(modules_dtype_dict=cfg.modules_dtype_dict, modules_to_not_use_matmul=cfg.modules_to_not_use_matmul,
                                        modules_to_not_convert=cfg.modules_to_not_convert))) == meta["lists"]
        for lname, info in meta["layers"].items():
            cands = [(d, m) for p, d, m in trace if p == info["param"]]
            ok &= [d for d, _ in cands] == info["candidates"] and [m for _, m in cands] == info["mse"]
            layer = getattr(model, lname)
            for k in ("weight", "scale", "zero_point", "svd_up", "svd_down"):
                key = f"{lname}.{k}"
                t = getattr(layer, k, None) if info["chosen"] != "float" else None
                if key in z.files:
                    a, _ = G.to_np(t)
                    ok &= a is not None and a.dtype == z[key].dtype and a.shape == z[key].shape and a.tobytes() == z[key].tobytes()
                else:
                    ok &= t is None
        bad += not ok
        print("verify", name, "OK" if ok else "MISMATCH")
    print("verify done, mismatching cases:", bad)
    return bad


def regen_check():
    """Regenerate every fixture into a temp dir and compare array by array with the tracked files."""
    import tempfile
    global OUT_DIR
    OUT_DIR = tempfile.mkdtemp(prefix="sdnq_golden_dyn_")
    generate(None)
    bad = 0
    for fn in sorted(os.listdir(OUT_DIR)):
        a, b = os.path.join(OUT_DIR, fn), os.path.join(HERE, fn)
        if not os.path.exists(b):
            print("regen-check: not tracked:", fn)
            bad += 1
        elif fn.endswith(".npz"):
            za, zb = np.load(a), np.load(b)
            same = sorted(za.files) == sorted(zb.files) and all(
                za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes() for k in za.files)
            bad += not same
            print("regen-check", fn, "identical" if same else "DIFFERS")
        else:
            same = open(a).read() == open(b).read()
            bad += not same
            print("regen-check", fn, "identical" if same else "DIFFERS")
    print("regen-check done, differing files:", bad, "(temp dir", OUT_DIR + ")")
    return bad


def generate(only):
    for c in CASES:
        if only is None or c["name"] in only:
            run_case(c)


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--verify" in sys.argv[1:]:
        sys.exit(1 if verify() else 0)
    if "--regen-check" in sys.argv[1:]:
        sys.exit(1 if regen_check() else 0)
    generate(sys.argv[1:] or None)
