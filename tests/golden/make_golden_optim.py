#!/usr/bin/env python3
"""Golden vectors for the fused AdamW step (sdnq_amd.optim, csrc/optim.hip), made by RUNNING the reference's `AdamW` (optim/adamw.py on
optim/optimizer.py and optim/utils.py) on the CPU for three consecutive steps of one parameter, with the environment switches and the
fake `diffusers` of make_golden.py and BOTH stochastic options off.  Files are ``optim_adamw_<name>.npz`` / ``.json`` (and, for
quantized state, ``optim_adamw_<name>_deq.npz`` with the dequantized values: together they would pass 1 MiB) and hold DATA only:

  p0, g1, g2, g3                              the parameter before the first step and the three gradients (the case's dtype)
  p1, p2, p3                                  the parameter after each step
  dense state:      exp_avg1..3, exp_avg_sq1..3                     in the parameter's dtype
  quantized state:  exp_avg_q1..3 (uint8 [R, G, 32]), exp_avg_scale1..3, exp_avg_zp1..3 (float32 [R, G, 1]), exp_avg_deq1..3 (float32,
                    SDNQTensor.dequantize()), and the same with exp_avg_sq
  the json: the options the optimizer was made with, `grad_scale` (a float, given to the optimizer as a float32 tensor) and what was
  planted in the gradients (and, for the cases with `planted_param`, in the parameter).
``optim_adamw_defaults.json`` records `SDNQOptimizer.apply_group_defaults({})` and the sorted `_group_keys` of the reference's AdamW.

Shapes are chosen against the geometry of csrc/optim.hip (a lane owns 8 elements, a block 2048, a uint8 group is four lanes):
[37, 24] = 888 elements (not a multiple of 8 x 64), [83] (a tail of 3), [130, 160] = 20 800 elements (>= the reference's 16 384 below
which state stays dense; 650 groups: not a whole number of 256-lane blocks), [2055] (one whole block and a tail of 7), [65, 64] = 4160
elements (two blocks and two groups; quantized_buffers_minimum_numel lowered to 1024).

Usage:  python tests/golden/make_golden_optim.py [case ...]
        python tests/golden/make_golden_optim.py --verify     # stored inputs -> the reference's AdamW -> stored outputs, bit for bit
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets the environment switches, installs the fake diffusers, imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdnq.optim import AdamW  # noqa: E402  (the reference)
from sdnq.optim.optimizer import SDNQOptimizer  # noqa: E402

STEPS = 3
# plants of the later cases, by flat index; "max" and "tiny" are the dtype's largest finite value and smallest subnormal.  Inside the
# first lane, across the lane boundary 7 | 8, and in the tail 2048..2054 of a [2055] tensor
PARAM_PLANTS = {1: "max", 2: "-0.0", 6: "inf", 7: "nan", 8: "-inf", 9: "tiny", 10: "-max",
                2048: "nan", 2049: "inf", 2050: "-0.0", 2051: "max", 2053: "tiny", 2054: "-inf"}
GRAD_PLANTS = {0: "nan", 3: "0.0", 4: "inf", 7: "tiny", 8: "-inf", 15: "nan", 16: "inf",
               2047: "0.0", 2048: "inf", 2052: "tiny", 2053: "nan", 2054: "0.0"}
Q8_GRAD_PLANTS = {0: "nan", 5: "inf", 8: "-inf", 31: "inf", 32: "nan", 2047: "inf", 2048: "nan", 4127: "-inf"}
CASES = [
    dict(name="dense_f32", dtype="f32", shape=(37, 24), opts=dict(lr=1e-3)),
    dict(name="dense_bf16_gradscale", dtype="bf16", shape=(37, 24), opts=dict(lr=0.05), grad_scale=3.0),
    dict(name="dense_f16_nonfinite", dtype="f16", shape=(37, 24), opts=dict(lr=0.02, weight_decay=0.1), nonfinite=True),
    dict(name="bias_bf16", dtype="bf16", shape=(83,), opts=dict(lr=0.05, betas=(0.8, 0.95))),
    dict(name="q8_f32_zero_group", dtype="f32", shape=(130, 160), opts=dict(lr=1e-3, use_quantized_buffers=True), zero_group=True),
    dict(name="q8_bf16_nodecay_nonorm", dtype="bf16", shape=(130, 160),
         opts=dict(lr=0.05, use_quantized_buffers=True, weight_decay=0.0, final_norm_mode="none")),
    # 1 - beta >= 0.5 (the other branch of lerp), a clip below 1, special values in the PARAMETER: [2055] is one block and a tail of 7
    dict(name="dense_f16_lowclip", dtype="f16", shape=(2055,), plants=True,
         opts=dict(lr=0.02, betas=(0.4, 0.3), clip_threshold=(0.25, 1e-3, 1e-3), weight_decay=0.0)),
    dict(name="dense_bf16_fastbetas", dtype="bf16", shape=(2055,), plants=True, opts=dict(betas=(0.4, 0.3))),
    # [65, 64] = 4160 elements: two blocks and two groups
    dict(name="q8_f16_fastbetas", dtype="f16", shape=(65, 64), grad_plants=Q8_GRAD_PLANTS, zero_group=[(64, 1)],
         opts=dict(lr=0.02, betas=(0.4, 0.3), clip_threshold=(0.25, 1e-3, 1e-3), use_quantized_buffers=True,
                   quantized_buffers_minimum_numel=1024)),
]
# where the special values go (flat indices / (row, group) pairs): inside the first lane, across a lane boundary and in the tail
NONFINITE = {0: float("nan"), 5: float("inf"), 8: float("-inf"), 401: float("inf"), 886: float("nan"), 887: float("-inf")}
ZERO_GROUPS = [(0, 0), (64, 2), (129, 4)]


def plant(t, plants):
    """Write `plants` ({flat index: name of a value}) into tensor `t` of the case's dtype, in place."""
    tiny = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}[t.dtype]
    named = {"max": torch.finfo(t.dtype).max, "tiny": tiny}
    flat = t.view(-1)
    for i, what in plants.items():
        mag = what.lstrip("-")
        flat[i] = (-1.0 if what.startswith("-") else 1.0) * (named[mag] if mag in named else float(mag))
    return t


def zero_groups_of(case):
    z = case.get("zero_group")
    return ZERO_GROUPS if z is True else (z or None)


def make_inputs(case):
    seed = zlib.crc32(("optim_adamw_" + case["name"]).encode())
    g = torch.Generator().manual_seed(seed)
    dt = G.TORCH_DT[case["dtype"]]
    shape = case["shape"]
    p0 = (torch.randn(*shape, generator=g) * 0.5).to(dt)
    if case.get("plants"):
        plant(p0, PARAM_PLANTS)
    grads = []
    for _ in range(STEPS):
        gr = torch.randn(*shape, generator=g) * 0.5 * (1.0 + torch.rand(*shape[:-1], 1, generator=g)) * case.get("grad_scale", 1.0)
        if case.get("nonfinite"):
            flat = gr.view(-1)
            for i, val in NONFINITE.items():
                flat[i] = val
        if case.get("zero_group"):
            for r, gi in zero_groups_of(case):
                gr[r, gi * 32:(gi + 1) * 32] = 0.0
        gr = gr.to(dt)
        if case.get("plants") or case.get("grad_plants"):
            plant(gr, case.get("grad_plants") or GRAD_PLANTS)
        grads.append(gr)
    return p0, grads


def run_reference(case, p0, grads):
    """{key: tensor} of everything the reference's AdamW leaves after each of the steps."""
    param = torch.nn.Parameter(p0.clone())
    opt = AdamW([param], use_stochastic_rounding=False, use_stochastic_buffers=False, **case["opts"])
    if "grad_scale" in case:
        opt.grad_scale = torch.tensor(case["grad_scale"], dtype=torch.float32)
    out = {}
    for i, gr in enumerate(grads, 1):
        param.grad = gr.clone()
        opt.step()
        state = opt.state[param]
        assert state["step"] == i
        out[f"p{i}"] = param.detach().clone()
        for key in ("exp_avg", "exp_avg_sq"):
            buf = state[key]
            if case["opts"].get("use_quantized_buffers"):
                assert type(buf).__name__ == "SDNQTensor" and buf.svd_up is None
                out[f"{key}_q{i}"] = buf.weight.detach().clone()
                out[f"{key}_scale{i}"] = buf.scale.detach().clone()
                out[f"{key}_zp{i}"] = buf.zero_point.detach().clone()
                out[f"{key}_deq{i}"] = buf.dequantize().detach().clone()
            else:
                assert type(buf) is torch.Tensor and buf.dtype == p0.dtype
                out[f"{key}{i}"] = buf.detach().clone()
    return out, opt.param_groups[0]


def jsonable(v):
    return list(v) if isinstance(v, tuple) else v


def run_case(case):
    p0, grads = make_inputs(case)
    res, group = run_reference(case, p0, grads)
    tensors = dict(p0=p0, **{f"g{i}": g for i, g in enumerate(grads, 1)}, **res)
    out, info = {}, {}
    for key, t in tensors.items():
        arr, tag = G.to_np(t)
        out[key] = arr
        info[key] = dict(dtype=tag, shape=list(t.shape))
    meta = dict(name=case["name"], dtype=case["dtype"], shape=list(case["shape"]), steps=STEPS,
                quantized=bool(case["opts"].get("use_quantized_buffers")), grad_scale=case.get("grad_scale"),
                options={k: jsonable(v) for k, v in group.items() if k != "params"},
                nonfinite={str(k): str(v) for k, v in NONFINITE.items()} if case.get("nonfinite") else None,
                zero_groups=zero_groups_of(case), tensors=info)
    if case.get("plants"):
        meta["planted_param"] = {str(k): v for k, v in PARAM_PLANTS.items()}
    if case.get("plants") or case.get("grad_plants"):
        meta["planted_grad"] = {str(k): v for k, v in (case.get("grad_plants") or GRAD_PLANTS).items()}
    # the dequantized values go to a file of their own: with them one file of a float32 [130, 160] case passes 1 MiB
    deq = {k: out.pop(k) for k in [k for k in out if "_deq" in k]}
    np.savez_compressed(os.path.join(HERE, f"optim_adamw_{case['name']}.npz"), **out)
    if deq:
        np.savez_compressed(os.path.join(HERE, f"optim_adamw_{case['name']}_deq.npz"), **deq)
    with open(os.path.join(HERE, f"optim_adamw_{case['name']}.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", case["name"], sorted(res))


def defaults():
    return dict(defaults={k: jsonable(v) for k, v in SDNQOptimizer.apply_group_defaults({}).items()}, group_keys=sorted(AdamW._group_keys))


def verify():
    bad = 0
    for case in CASES:
        name = case["name"]
        with open(os.path.join(HERE, f"optim_adamw_{name}.json")) as f:
            meta = json.load(f)
        z = dict(np.load(os.path.join(HERE, f"optim_adamw_{name}.npz")))
        if meta["quantized"]:
            z.update(np.load(os.path.join(HERE, f"optim_adamw_{name}_deq.npz")))
        t = {k: G.from_np(z[k], i["dtype"]).reshape(i["shape"]) for k, i in meta["tensors"].items()}
        res, _ = run_reference(case, t["p0"], [t[f"g{i}"] for i in range(1, STEPS + 1)])
        for key, r in res.items():
            # bit patterns: NaN-free by construction, but -0.0 and 0.0 must not pass for each other
            ok = key in t and r.dtype == t[key].dtype and np.array_equal(G.to_np(r)[0], G.to_np(t[key])[0])
            bad += not ok
            if not ok:
                print("verify", name, key, "MISMATCH")
        print("verify", name, len(res), "tensors")
    with open(os.path.join(HERE, "optim_adamw_defaults.json")) as f:
        ok = json.load(f) == json.loads(json.dumps(defaults()))
    bad += not ok
    print("verify defaults", "OK" if ok else "MISMATCH")
    print("verify done, mismatches:", bad)
    return bad


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--verify" in sys.argv[1:]:
        sys.exit(1 if verify() else 0)
    only = sys.argv[1:]
    for c in CASES:
        if not only or c["name"] in only:
            run_case(c)
    if not only:
        with open(os.path.join(HERE, "optim_adamw_defaults.json"), "w") as f:
            json.dump(defaults(), f, indent=1)
