#!/usr/bin/env python3
"""Golden vectors for the int8 training Linear (sdnq_amd.training), made by RUNNING the reference's two autograd functions on the CPU --
`int8_matmul_dynamic_with_backward` (training/layers/linear/linear_int8/linear_int8_dynamic.py) and `int8_matmul_dynamic_with_backward_ckpt`
(linear_int8_dynamic_ckpt.py) -- with the environment switches and the fake `diffusers` of make_golden.py.  Files are
``train_int8_<name>.npz`` / ``.json`` and hold DATA only:

  x, w, bias, dy                               the inputs (dy = grad_output)
  y, grad_input, grad_weight, grad_bias        the reference's results (absent where the case's `need` does not ask for a gradient)
  the six quantizations, from quantize_int_mm on the same tensors with the `dim` the functions use, in the reference's own orientation:
    fwd_x_q  [M][K], fwd_x_s  [M][1]           quantize_int_mm(x2d, dim=-1)
    fwd_w_q  [K][N], fwd_w_s  [1][N]           quantize_int_mm(w.t(), dim=0)            (one scale per output row)
    gi_dy_q  [M][N], gi_dy_s  [M][1]           quantize_int_mm(dy2d, dim=-1)
    gi_w_q   [N][K], gi_w_s   [1][K]           quantize_int_mm(w, dim=0)                (one scale per input channel)
    gw_dy_q  [N][M], gw_dy_s  [N][1]           quantize_int_mm(dy2d.t(), dim=-1)
    gw_x_q   [M][K], gw_x_s   [1][K]           quantize_int_mm(x2d, dim=0)
The ckpt function's results are required to equal the plain function's bit for bit before anything is written (meta "ckpt_identical").

Shapes (M 33..300, N 48..96, K 64..128) are chosen against the geometry of csrc/colquant.hip: 64-column tiles (48, 80, 96 are not
multiples), 128-row statistics slabs and 256-row quantize tiles (M = 300 spans three and two of them), M not a multiple of 16 (33, 72).
No input has an all-zero column (the reference's result there is a NaN cast to int8).  `ties` is constructed: columns of exact rounding
ties (k + 0.5) and their one-ulp neighbours, after tests/test_gpu_parity.py's tie rows.

Usage:  python tests/golden/make_golden_training.py [case ...]
        python tests/golden/make_golden_training.py --verify     # stored inputs -> reference functions -> stored outputs, bit for bit
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
from sdnq.quant_utils import quantize_int_mm  # noqa: E402  (the reference)
from sdnq.training.layers.linear.linear_int8.linear_int8_dynamic import int8_matmul_dynamic_with_backward  # noqa: E402
from sdnq.training.layers.linear.linear_int8.linear_int8_dynamic_ckpt import int8_matmul_dynamic_with_backward_ckpt  # noqa: E402

ALL = (True, True, True)
CASES = [
    dict(name="bf16_m33", dtype="bf16", lead=(33,), K=64, N=48, bias=True),
    dict(name="bf16_m72_3d", dtype="bf16", lead=(2, 36), K=128, N=96, bias=True),
    dict(name="bf16_m300", dtype="bf16", lead=(300,), K=80, N=64, bias=True),
    dict(name="f16_m72_nobias", dtype="f16", lead=(72,), K=64, N=48, bias=False),
    dict(name="f16_m300_3d", dtype="f16", lead=(3, 100), K=96, N=80, bias=True),
    dict(name="f32_m33_nobias", dtype="f32", lead=(33,), K=128, N=64, bias=False),
    dict(name="f32_m200", dtype="f32", lead=(200,), K=80, N=96, bias=True),
    dict(name="bf16_m130_input_only", dtype="bf16", lead=(130,), K=64, N=80, bias=True, need=(True, False, False)),
    dict(name="f16_m130_weight_only", dtype="f16", lead=(130,), K=96, N=48, bias=True, need=(False, True, False)),
    dict(name="bf16_m72_no_bias_grad", dtype="bf16", lead=(72,), K=64, N=64, bias=True, need=(True, True, False)),
    dict(name="ties", dtype="f32", lead=(144,), K=64, N=64, bias=True, ties=True),
]


def tie_matrix(rows, cols, rng):
    """[rows][cols] float32: column c has amax 127 s_c (first row) over exact ties (k + 0.5) s_c; odd columns sit one ulp beside them."""
    out = np.empty((rows, cols), dtype=np.float32)
    scales = (1.0, 2.0, 0.5, 1.5, 3.0, 0.75, 1.25, 6.0)
    for c in range(cols):
        s = scales[c % len(scales)]
        col = ((rng.integers(-126, 126, size=rows) + 0.5) * s).astype(np.float32)  # exact in float32
        if c % 2:
            col = np.nextafter(col, (np.float32(np.inf) * np.sign(rng.standard_normal(rows))).astype(np.float32))
        col[0] = 127.0 * s
        out[:, c] = col
    return torch.from_numpy(out)


def make_inputs(case):
    seed = zlib.crc32(("train_int8_" + case["name"]).encode())
    g = torch.Generator().manual_seed(seed)
    dt = G.TORCH_DT[case["dtype"]]
    m = int(np.prod(case["lead"]))
    k, n = case["K"], case["N"]
    if case.get("ties"):
        rng = np.random.default_rng(seed)
        x, w, dy = tie_matrix(m, k, rng), tie_matrix(n, k, rng) * 0.01, tie_matrix(m, n, rng) * 0.125
    else:
        x = torch.randn(m, k, generator=g) * (1.0 + 3.0 * torch.rand(1, k, generator=g))  # uneven channels
        w = torch.randn(n, k, generator=g) * 0.05
        dy = torch.randn(m, n, generator=g) * 0.02 * (1.0 + 2.0 * torch.rand(m, 1, generator=g))
    bias = (torch.randn(n, generator=g) * 0.1).to(dt) if case["bias"] else None
    return x.to(dt).reshape(*case["lead"], k), w.to(dt), bias, dy.to(dt).reshape(*case["lead"], n)


def run_reference(fn, x, w, bias, dy, need):
    x, w = x.clone().requires_grad_(need[0]), w.clone().requires_grad_(need[1])
    b = bias.clone().requires_grad_(need[2]) if bias is not None else None
    y = fn(x, w, b)
    y.backward(dy)
    return y.detach(), x.grad, w.grad, (b.grad if b is not None else None)


def quantizations(x, w, dy):
    x2d, g2d = x.flatten(0, -2).float(), dy.flatten(0, -2).float()
    wf = w.float()
    out = {}
    for key, (t, dim) in {"fwd_x": (x2d, -1), "fwd_w": (wf.t(), 0), "gi_dy": (g2d, -1), "gi_w": (wf, 0), "gw_dy": (g2d.t(), -1),
                          "gw_x": (x2d, 0)}.items():
        q, s = quantize_int_mm(t, dim=dim)
        out[key + "_q"], out[key + "_s"] = q.contiguous(), s.contiguous()
    return out


def count_ties(x2d, dim):
    x2d = x2d.float()
    quot = x2d / (x2d.abs().amax(dim=dim, keepdim=True) / 127)
    return int(((quot - torch.floor(quot)) == 0.5).sum())


def run_case(case):
    need = tuple(case.get("need", ALL))
    if not case["bias"]:
        need = (need[0], need[1], False)
    x, w, bias, dy = make_inputs(case)
    with torch.enable_grad():
        res = run_reference(int8_matmul_dynamic_with_backward, x, w, bias, dy, need)
        res_ckpt = run_reference(int8_matmul_dynamic_with_backward_ckpt, x, w, bias, dy, need)
    for a, b in zip(res, res_ckpt):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (case["name"], "ckpt differs from the plain function")
    tensors = dict(x=x, w=w, dy=dy, y=res[0])
    if bias is not None:
        tensors["bias"] = bias
    for key, t in zip(("grad_input", "grad_weight", "grad_bias"), res[1:]):
        if t is not None:
            tensors[key] = t
    tensors.update(quantizations(x, w, dy))
    assert all(float(t.float().abs().amax(0).min()) > 0 for t in (x.flatten(0, -2), w, dy.flatten(0, -2))), "an all-zero column"
    out, info = {}, {}
    for key, t in tensors.items():
        arr, tag = G.to_np(t)
        out[key] = arr
        info[key] = dict(dtype=tag, shape=list(t.shape))
    meta = dict(name=case["name"], dtype=case["dtype"], M=int(np.prod(case["lead"])), N=case["N"], K=case["K"], need=list(need),
                ckpt_identical=True, tensors=info,
                ties=dict(gw_x=count_ties(x.flatten(0, -2), 0), gi_w=count_ties(w, 0), gw_dy=count_ties(dy.flatten(0, -2), 0)))
    np.savez_compressed(os.path.join(HERE, f"train_int8_{case['name']}.npz"), **out)
    with open(os.path.join(HERE, f"train_int8_{case['name']}.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", case["name"], "M", meta["M"], "ties", meta["ties"])


def verify():
    bad = 0
    for case in CASES:
        name = case["name"]
        with open(os.path.join(HERE, f"train_int8_{name}.json")) as f:
            meta = json.load(f)
        z = np.load(os.path.join(HERE, f"train_int8_{name}.npz"))
        t = {k: G.from_np(z[k], i["dtype"]).reshape(i["shape"]) for k, i in meta["tensors"].items()}
        for fn in (int8_matmul_dynamic_with_backward, int8_matmul_dynamic_with_backward_ckpt):
            with torch.enable_grad():
                res = run_reference(fn, t["x"], t["w"], t.get("bias"), t["dy"], tuple(meta["need"]))
            for key, r in zip(("y", "grad_input", "grad_weight", "grad_bias"), res):
                ok = (r is None and key not in t) or (r is not None and key in t and torch.equal(r, t[key]))
                bad += not ok
                print("verify", name, fn.__self__.__name__ if hasattr(fn, "__self__") else "", key, "OK" if ok else "MISMATCH")
        for key, r in quantizations(t["x"], t["w"], t["dy"]).items():
            ok = torch.equal(r, t[key])
            bad += not ok
            if not ok:
                print("verify", name, key, "MISMATCH")
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
