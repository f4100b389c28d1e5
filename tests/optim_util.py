"""A float64 restatement, in torch on the CPU, of one AdamW step as the reference's optimizer chains it (optim/optimizer.py step ->
get_param_grad -> adam_update -> apply_norm_to_update_ -> update_param_ -> copy_stochastic_), the loading of the fixtures
tests/golden/optim_adamw_* (tests/golden/make_golden_optim.py) and the error measures the optimizer tests share.

    g = clamp(nan_to_num(grad) / grad_scale, -clip, clip)            nan_to_num in the gradient's dtype, as nan_to_num_() on param.grad
    m = m + (1 - beta1) (g - m) ;  v = v + (1 - beta2) (g g - v)
    u = clamp(nan_to_num((m / (1 - beta1^t)) rsqrt(v / (1 - beta2^t))), -clip, clip)            ("none" and "clip" add nothing after this)
    p = nan_to_num(p) (1 - lr wd) - lr u
    storage: p, and dense m, v, rounded to the parameter's dtype; quantized m, v as uint8 codes per group of 32 along the last
    dimension: zero point = min, scale = (max - min) / 255 (both stored in float32), code = round_half_even((x - min) / scale), an
    all-equal group: scale 0 and codes 0.
Every scalar (1 - beta, 1 - beta^t, 1 - lr wd) is the Python double; nothing is rounded to float32 in between.

Error measure of the tests: distance(a, ref) = max |a - ref| / max |ref| per tensor.  `REL_ULP[dtype]` is one unit in the last place of
the dtype relative to a power of two: the largest relative size of one ulp at the tensor's magnitude scale.

At the end: the fixtures through the float32 oracle (oracle/oracle.py: adamw_step, adamw_step_q8), which reproduces them bit for bit
(tests/test_optim_oracle.py) and which tests/test_optim_exact_gpu.py holds the kernel to.
"""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
REL_ULP = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10, "f32": 2.0 ** -23}
# float32 roundings between the inputs and any stored value of the chain, each at most half an ulp of a value no larger than the
# clip-bounded tensors they build: lerp (2: the difference, the fma), bias correction (2), rsqrt and product (2), decay and update (2)
CHAIN_ROUNDINGS = 8
F32_CHAIN = CHAIN_ROUNDINGS * 2.0 ** -24
GROUP = 32
STEPS = 3


def names():
    return sorted(f[len("optim_adamw_"):-5] for f in os.listdir(GOLD)
                  if f.startswith("optim_adamw_") and f.endswith(".json") and f != "optim_adamw_defaults.json")


def recorded_defaults():
    return json.load(open(os.path.join(GOLD, "optim_adamw_defaults.json")))


_CACHE = {}


def load(name):
    """(meta, {key: tensor}) of one fixture, loaded once and shared (treat the tensors as read-only); 16-bit floats in their dtype."""
    if name not in _CACHE:
        meta = json.load(open(os.path.join(GOLD, f"optim_adamw_{name}.json")))
        z = dict(np.load(os.path.join(GOLD, f"optim_adamw_{name}.npz")))
        if meta["quantized"]:
            z.update(np.load(os.path.join(GOLD, f"optim_adamw_{name}_deq.npz")))
        out = {}
        for key, info in meta["tensors"].items():
            t = torch.from_numpy(np.ascontiguousarray(z[key]))
            if info["dtype"] in ("bf16", "f16"):
                t = t.view(TORCH_DT[info["dtype"]])
            out[key] = t.reshape(info["shape"])
        _CACHE[name] = (meta, out)
    return _CACHE[name]


def state_before(meta, t, i):
    """The optimizer state the fixture holds in front of step i (1-based): {key: tensor}, zeros in front of step 1."""
    shape = meta["shape"]
    if not meta["quantized"]:
        if i == 1:
            z = torch.zeros(shape, dtype=TORCH_DT[meta["dtype"]])
            return dict(exp_avg=z, exp_avg_sq=z.clone())
        return dict(exp_avg=t[f"exp_avg{i - 1}"], exp_avg_sq=t[f"exp_avg_sq{i - 1}"])
    out = {}
    for key in ("exp_avg", "exp_avg_sq"):
        if i == 1:
            g = shape[-1] // GROUP
            out[key + "_q"] = torch.zeros(*shape[:-1], g, GROUP, dtype=torch.uint8)
            out[key + "_scale"] = torch.zeros(*shape[:-1], g, 1)
            out[key + "_zp"] = torch.zeros(*shape[:-1], g, 1)
        else:
            for part in ("_q", "_scale", "_zp"):
                out[key + part] = t[f"{key}{part}{i - 1}"]
    return out


def quantize64(x, shape):
    """(codes uint8 [.., G, 32], scale f32 [.., G, 1], zero point f32 [.., G, 1], dequantized f64 of `shape`) of a float64 tensor."""
    xg = x.reshape(*shape[:-1], shape[-1] // GROUP, GROUP)
    lo, hi = xg.amin(-1, keepdim=True), xg.amax(-1, keepdim=True)
    scale = (hi - lo) / 255.0
    q = torch.where(scale == 0, torch.zeros_like(xg), torch.round((xg - lo) / scale)).clamp(0, 255)
    scale32, zp32 = scale.float(), lo.float()
    return q.to(torch.uint8), scale32, zp32, (zp32.double() + q * scale32.double()).reshape(shape)


def restate(meta, p_prev, grad, state, step):
    """One step in float64.  `state`: as state_before returns it.  Returns {key: tensor} with the fixture's keys without the step
    number: p and exp_avg / exp_avg_sq rounded to the dtype (dense), or exp_avg_q / _scale / _zp / _deq (quantized)."""
    o = meta["options"]
    dt = TORCH_DT[meta["dtype"]]
    clips = o["clip_threshold"]
    clip = clips if isinstance(clips, (int, float)) else clips[0]
    b1, b2 = o["betas"]
    lr, wd = o["lr"], o["weight_decay"]
    assert o["final_norm_mode"] in ("clip", "none")
    g = torch.nan_to_num(grad).double()
    if meta["grad_scale"] is not None:
        g = g / float(np.float32(meta["grad_scale"]))
    g = g.clamp(-clip, clip)
    p = torch.nan_to_num(p_prev).double()
    if meta["quantized"]:
        m, v = ((state[k + "_zp"].double() + state[k + "_q"].double() * state[k + "_scale"].double()).reshape(meta["shape"])
                for k in ("exp_avg", "exp_avg_sq"))
    else:
        m, v = state["exp_avg"].double(), state["exp_avg_sq"].double()
    m = m + (1.0 - b1) * (g - m)
    v = v + (1.0 - b2) * (g * g - v)
    u = (m / (1.0 - b1 ** step)) * torch.rsqrt(v / (1.0 - b2 ** step))
    u = torch.nan_to_num(u, posinf=float(np.finfo(np.float32).max), neginf=-float(np.finfo(np.float32).max)).clamp(-clip, clip)
    if wd != 0:
        p = p * (1.0 - lr * wd)
    p = p - lr * u
    out = dict(p=p.to(dt))
    if meta["quantized"]:
        for key, x in (("exp_avg", m), ("exp_avg_sq", v)):
            out[key + "_q"], out[key + "_scale"], out[key + "_zp"], out[key + "_deq"] = quantize64(x, meta["shape"])
    else:
        out["exp_avg"], out["exp_avg_sq"] = m.to(dt), v.to(dt)
    out["exp_avg_f64"], out["exp_avg_sq_f64"], out["p_f64"] = m, v, p
    return out


def restate_fixture_step(name, i):
    """Step i of fixture `name` restated from the fixture's own state in front of it."""
    meta, t = load(name)
    return restate(meta, t[f"p{i - 1}"], t[f"g{i}"], state_before(meta, t, i), i)


def distance(a, ref):
    a, ref = a.double(), ref.double()
    top = ref.abs().max().item()
    return 0.0 if top == 0 and torch.equal(a, ref) else (a - ref).abs().max().item() / top if top else float("inf")


def ulps_f32(a, b):
    """Largest distance of two float32 tensors in units in the last place (finite values of one sign pattern or zeros)."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return (ia - ib).abs().max().item()


def reference_distances(name):
    """{(key, step): distance of the reference's stored result from the restatement}: p and the state tensors that are stored as
    floats; for quantized state also ("code_share", key, step): the share of codes that differ."""
    meta, t = load(name)
    out = {}
    for i in range(1, STEPS + 1):
        r = restate_fixture_step(name, i)
        keys = ("p", "exp_avg_deq", "exp_avg_sq_deq") if meta["quantized"] else ("p", "exp_avg", "exp_avg_sq")
        for key in keys:
            out[(key, i)] = distance(r[key], t[f"{key}{i}"])
        if meta["quantized"]:
            for key in ("exp_avg", "exp_avg_sq"):
                out[("code_share", key, i)] = (r[key + "_q"] != t[f"{key}_q{i}"]).double().mean().item()
    return out


def deq_excess(deq, ref_deq, ref_scale, shape):
    """How many dequantized elements lie further than one quantization step (their group's scale in the fixture) from the fixture's.
    Slack beside the step: the float32 roundings of a dequantized value (half an ulp), of its zero point and of its scale (up to 2 ulp
    each in the tests, the scale multiplied by a code of up to 255) -- under 2^-20 of the larger of |value| and the group's range."""
    g = shape[-1] // GROUP
    step = ref_scale.double().reshape(*shape[:-1], g, 1).expand(*shape[:-1], g, GROUP).reshape(shape)
    ref = ref_deq.double().reshape(shape)
    slack = 2.0 ** -20 * torch.maximum(ref.abs(), 255.0 * step)
    return int(((deq.double().reshape(shape) - ref).abs() > step + slack).sum())


# ---- the float32 oracle (oracle/oracle.py: adamw_step, adamw_step_q8) on the fixtures -----------------------------------------------------
def f32_array(t):
    """A float tensor of any of the three dtypes as a flat float32 ndarray (exact)."""
    return t.detach().cpu().float().contiguous().view(-1).numpy()


def bit_array(t):
    """The bit patterns of a tensor, flat: uint16 / uint32 / uint8 ndarray (so that -0.0 differs from 0.0 and a NaN compares)."""
    t = t.detach().cpu().contiguous().view(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def stored_bits(x, tag):
    """The bits that a deterministic store of float32 ndarray `x` to dtype `tag` leaves (oracle.round_dtype's rounding)."""
    from oracle import oracle as O
    return O.to_bits(x, tag).view(np.uint32 if tag == "f32" else np.uint16).reshape(-1)


def oracle_options(meta, i):
    """The keyword arguments of oracle.adamw_step / sdnq_amd.ops.adamw_step for step i of a fixture."""
    o = meta["options"]
    clips = o["clip_threshold"]
    return dict(step=i, lr=o["lr"], betas=tuple(o["betas"]), weight_decay=o["weight_decay"],
                clip=clips if isinstance(clips, (int, float)) else clips[0], grad_scale=meta["grad_scale"])


_ORACLE = {}


def oracle_fixture_step(name, i):
    """Step i of fixture `name` by the float32 oracle, from the fixture's own state in front of it: what oracle.adamw_step /
    adamw_step_q8 return (flat float32 ndarrays, unrounded).  Computed once and shared: treat as read-only."""
    if (name, i) not in _ORACLE:
        from oracle import oracle as O
        meta, t = load(name)
        s = state_before(meta, t, i)
        p, g = f32_array(t[f"p{i - 1}"]), f32_array(t[f"g{i}"])
        if meta["quantized"]:
            st = [(s[k + "_q"].reshape(-1).numpy(), s[k + "_scale"].reshape(-1).numpy(), s[k + "_zp"].reshape(-1).numpy())
                  for k in ("exp_avg", "exp_avg_sq")]
            _ORACLE[(name, i)] = O.adamw_step_q8(p, g, st[0], st[1], meta["dtype"], **oracle_options(meta, i))
        else:
            _ORACLE[(name, i)] = O.adamw_step(p, g, f32_array(s["exp_avg"]), f32_array(s["exp_avg_sq"]), meta["dtype"],
                                              **oracle_options(meta, i))
    return _ORACLE[(name, i)]
