"""The multi-tensor AdamW step on the MI355X (csrc/optim.hip: adamw_dense_multi_kernel, adamw_q8_multi_kernel) against the
single-tensor entry points: every parameter, state tensor, scale and zero point has the BITS of ops.adamw_step / ops.adamw_step_q8 run
tensor by tensor with the same step, seed and offset -- deterministic and stochastic alike -- and nothing outside the tensors is
written.  Sizes: around the lane (8 elements), the tail lane and the block (2048); counts: around the capacity of one launch
(sdnq_hip_adamw_multi_capacity).  The tensors of a case are carved out of one arena per role, 16-byte-multiple gaps of a sentinel byte
between them, so a block that strays into a neighbour or a gap shows.  Deterministic float32 cases are also held to the float32 oracle
by the rule of tests/test_optim_exact_gpu.py (state: the oracle's bits; parameter: within its rsqrt interval)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as U  # noqa: E402
from test_optim_exact_gpu import Tally, param_rule, same_bits  # noqa: E402

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAGS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = 0xA5
DENSE_NUMELS = [1, 7, 8, 9, 2047, 2048, 2049, 4101]
Q8_NUMELS = [32, 64, 2016, 2048, 2080, 4128]
MODES = [(False, False), (True, False), (False, True)]  # (sr_param, sr_state)
KW = dict(lr=0.02, betas=(0.9, 0.999), weight_decay=0.1, clip=1.0)
SEED = 0x123456789ABCDEF0
GS = 3.0


def _ops():
    from sdnq_amd import ops
    return ops


def capacity(quantized):
    from sdnq_amd import _lib
    return _lib.load().sdnq_hip_adamw_multi_capacity(int(quantized))


def counts(quantized):
    cap = capacity(quantized)
    return [1, 2, cap, cap + 1, 2 * cap + 3]


class Arena:
    """Tensors of the given flat values (a list of CPU tensors of one dtype) inside ONE device allocation filled with a sentinel byte:
    every tensor starts 16-byte aligned and is followed by the sentinel up to the next multiple of 16 and by a gap of 16, 32 or 48 more."""

    def __init__(self, values):
        self.spans, at = [], 48
        for k, x in enumerate(values):
            nbytes = x.numel() * x.element_size()
            self.spans.append((at, nbytes, x.dtype))
            at += (nbytes + 15) // 16 * 16 + 16 * (1 + k % 3)
        host = torch.full((at,), SENTINEL, dtype=torch.uint8)
        self.guard = torch.ones(at, dtype=torch.bool)
        for (start, nbytes, _), x in zip(self.spans, values):
            host[start:start + nbytes] = x.contiguous().view(-1).view(torch.uint8)
            self.guard[start:start + nbytes] = False
        self.guard = self.guard.to(DEV)
        self.buf = host.to(DEV)
        assert self.buf.data_ptr() % 16 == 0

    def views(self, buf=None):
        buf = self.buf if buf is None else buf
        return [buf[start:start + nbytes].view(dt) for start, nbytes, dt in self.spans]

    def guards_intact(self):
        return bool((self.buf[self.guard] == SENTINEL).all())


def _steps_and_offsets(count):
    """Per tensor: a first step in 1..5 and a Philox offset of its own, some above 2^32."""
    return [1 + k % 5 for k in range(count)], [(3 + 5 * k) if k % 4 else (1 << 32) + 12 + k for k in range(count)]


def _dense_case(numels, dt, seed):
    g = torch.Generator().manual_seed(seed)
    roles = {"p": [], "g": [], "m": [], "v": []}
    for n in numels:
        roles["p"].append((torch.randn(n, generator=g) * 0.5).to(dt))
        roles["g"].append((torch.randn(n, generator=g) * 1.5).to(dt))
        roles["m"].append((torch.randn(n, generator=g) * 0.1).to(dt))
        roles["v"].append((torch.rand(n, generator=g) * 0.1).to(dt))
    return {k: Arena(v) for k, v in roles.items()}


@pytest.mark.parametrize("count_index", range(5), ids=["1", "2", "cap", "cap+1", "2cap+3"])
@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
def test_dense_state_has_the_bits_of_the_single_tensor_step(tag, count_index):
    ops, dt = _ops(), TAGS[tag]
    count = counts(False)[count_index]
    numels = [DENSE_NUMELS[k % len(DENSE_NUMELS)] for k in range(count)]
    first, offsets = _steps_and_offsets(count)
    gs = torch.tensor([GS], dtype=torch.float32, device=DEV)
    tally = Tally()
    for with_gs in (False, True):
        for sr_param, sr_state in MODES:
            A = _dense_case(numels, dt, 100 + count)
            ref = {k: a.buf.clone() for k, a in A.items()}          # the single-tensor twin's arenas
            grads = A["g"].buf.clone()
            kw = dict(grad_scale=gs if with_gs else None, sr_param=sr_param, sr_state=sr_state, seed=SEED, **KW)
            for s in (0, 1):
                steps = [f + s for f in first]
                before = {k: ref[k].cpu() for k in "pmv"} if tag == "f32" and not (sr_param or sr_state) else None
                ops.adamw_step_multi(A["p"].views(), A["g"].views(), A["m"].views(), A["v"].views(), steps=steps, offsets=offsets, **kw)
                for p, g, m, v, step, offset in zip(*(A[k].views(ref[k]) for k in "pgmv"), steps, offsets):
                    ops.adamw_step(p, g, m, v, step=step, offset=offset, **kw)
                torch.cuda.synchronize()
                what = (tag, count, with_gs, sr_param, sr_state, s)
                for k in "pmv":
                    assert torch.equal(A[k].buf, ref[k]), what + (k,)
                    assert A[k].guards_intact(), what + (k, "guard")
                assert torch.equal(A["g"].buf, grads), what + ("gradient",)
                if before is not None:
                    old = {k: A[k].views(before[k]) for k in "pmv"}
                    new = {k: A[k].views(A[k].buf.cpu()) for k in "pmv"}
                    gcpu = A["g"].views(grads.cpu())
                    for i, step in enumerate(steps):
                        r = O.adamw_step(*(U.f32_array(x[i]) for x in (old["p"], gcpu, old["m"], old["v"])), tag, step=step,
                                         grad_scale=GS if with_gs else None, **KW)
                        same_bits(new["m"][i], U.stored_bits(r["exp_avg"], tag), what + (i, "exp_avg"))
                        same_bits(new["v"][i], U.stored_bits(r["exp_avg_sq"], tag), what + (i, "exp_avg_sq"))
                        param_rule(new["p"][i], r, tag, KW["lr"], KW["clip"], tally, what=what + (i,))
    if tag == "f32":
        print(f"multi dense x{count}: largest float32 distance of a parameter from the oracle {tally.dist:.3f} tol")


def _q8_case(numels, dt, seed):
    g = torch.Generator().manual_seed(seed)
    roles = {k: [] for k in ("p", "g", "mq", "ms", "mz", "vq", "vs", "vz")}
    for n in numels:
        roles["p"].append((torch.randn(n, generator=g) * 0.5).to(dt))
        roles["g"].append((torch.randn(n, generator=g) * 1.5).to(dt))
        roles["mq"].append(torch.randint(0, 256, (n,), generator=g).to(torch.uint8))
        roles["ms"].append(torch.rand(n // 32, generator=g) * 1e-3)
        roles["mz"].append(torch.rand(n // 32, generator=g) * -0.1)
        roles["vq"].append(torch.randint(0, 256, (n,), generator=g).to(torch.uint8))
        roles["vs"].append(torch.rand(n // 32, generator=g) * 1e-4)
        roles["vz"].append(torch.rand(n // 32, generator=g) * 0.01)
    return {k: Arena(v) for k, v in roles.items()}


STATE = ("mq", "ms", "mz", "vq", "vs", "vz")


@pytest.mark.parametrize("count_index", range(5), ids=["1", "2", "cap", "cap+1", "2cap+3"])
@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
def test_uint8_state_has_the_bits_of_the_single_tensor_step(tag, count_index):
    ops, dt = _ops(), TAGS[tag]
    count = counts(True)[count_index]
    numels = [Q8_NUMELS[k % len(Q8_NUMELS)] for k in range(count)]
    first, offsets = _steps_and_offsets(count)
    gs = torch.tensor([GS], dtype=torch.float32, device=DEV)
    tally = Tally()
    written = ("p",) + STATE
    for with_gs in (False, True):
        for sr_param, sr_state in MODES:
            A = _q8_case(numels, dt, 200 + count)
            ref = {k: a.buf.clone() for k, a in A.items()}
            grads = A["g"].buf.clone()
            kw = dict(grad_scale=gs if with_gs else None, sr_param=sr_param, sr_state=sr_state, seed=SEED, **KW)
            for s in (0, 1):
                steps = [f + s for f in first]
                before = {k: ref[k].cpu() for k in written} if tag == "f32" and not (sr_param or sr_state) else None
                cols = {k: A[k].views() for k in A}
                ops.adamw_step_multi_q8(cols["p"], cols["g"], list(zip(cols["mq"], cols["ms"], cols["mz"])),
                                        list(zip(cols["vq"], cols["vs"], cols["vz"])), steps=steps, offsets=offsets, **kw)
                rc = {k: A[k].views(ref[k]) for k in A}
                for i, (step, offset) in enumerate(zip(steps, offsets)):
                    ops.adamw_step_q8(rc["p"][i], rc["g"][i], (rc["mq"][i], rc["ms"][i], rc["mz"][i]), (rc["vq"][i], rc["vs"][i], rc["vz"][i]),
                                      step=step, offset=offset, **kw)
                torch.cuda.synchronize()
                what = (tag, count, with_gs, sr_param, sr_state, s)
                for k in written:
                    assert torch.equal(A[k].buf, ref[k]), what + (k,)
                    assert A[k].guards_intact(), what + (k, "guard")
                assert torch.equal(A["g"].buf, grads), what + ("gradient",)
                if before is not None:
                    old = {k: A[k].views(before[k]) for k in written}
                    new = {k: A[k].views(A[k].buf.cpu()) for k in written}
                    gcpu = A["g"].views(grads.cpu())
                    for i, step in enumerate(steps):
                        r = O.adamw_step_q8(U.f32_array(old["p"][i]), U.f32_array(gcpu[i]), tuple(old[k][i].numpy() for k in STATE[:3]),
                                            tuple(old[k][i].numpy() for k in STATE[3:]), tag, step=step,
                                            grad_scale=GS if with_gs else None, **KW)
                        for key, (q, sc, zp) in (("exp_avg", STATE[:3]), ("exp_avg_sq", STATE[3:])):
                            same_bits(new[q][i], r[key + "_q"], what + (i, key, "codes"))
                            same_bits(new[sc][i], r[key + "_scale"].view(np.uint32), what + (i, key, "scale"))
                            same_bits(new[zp][i], r[key + "_zp"].view(np.uint32), what + (i, key, "zero point"))
                        param_rule(new["p"][i], r, tag, KW["lr"], KW["clip"], tally, what=what + (i,))
    if tag == "f32":
        print(f"multi uint8 x{count}: largest float32 distance of a parameter from the oracle {tally.dist:.3f} tol")


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _state_bits(opt, p):
    out = [bits(p.detach()).clone()]
    for key in ("exp_avg", "exp_avg_sq"):
        x = opt.state[p].get(key)
        if x is not None:
            out += [bits(t).clone() for t in (x.parts() if hasattr(x, "parts") else (x,))]
    return out


def _adapter_model():
    """[(group, shape, dtype)] of 2 * cap + 5 tensors modelled on adapters: group 0 dense state, group 1 quantized state for its 2-D
    tensors of at least 512 elements; the bf16 dense bucket of group 0 alone is longer than one launch."""
    cap = capacity(False)
    bf, f32 = torch.bfloat16, torch.float32
    shapes = [(16, 64), (64, 16), (5,), (33,)]
    spec = [(0, shapes[k % 4], bf) for k in range(cap + 2)] + [(0, shapes[k % 4], f32) for k in range(cap + 3 - 46)]
    spec += [(1, (32, 64) if k % 2 else (16, 64), bf) for k in range(20)] + [(1, (32, 64), f32)]
    spec += [(1, (33,) if k % 2 else (5,), bf) for k in range(24)] + [(1, (5,), f32)]
    assert len(spec) == 2 * cap + 5
    return spec


def _run_optimizer(multi, monkeypatch, calls):
    from sdnq_amd import optim
    monkeypatch.setattr(optim, "MULTI", multi)
    spec = _adapter_model()
    g = torch.Generator().manual_seed(77)
    p0 = [(torch.randn(*shape, generator=g) * 0.5).to(dt) for _, shape, dt in spec]
    grads = [[(torch.randn(*shape, generator=g) * 0.4).to(dt) for _, shape, dt in spec] for _ in range(3)]
    params = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    groups = [dict(params=[p for p, s in zip(params, spec) if s[0] == 0], lr=1e-2, weight_decay=0.1),
              dict(params=[p for p, s in zip(params, spec) if s[0] == 1], lr=5e-3, weight_decay=0.0, use_quantized_buffers=True,
                   quantized_buffers_minimum_numel=512)]
    opt = optim.AdamW(groups)
    assert opt.param_groups[0]["use_stochastic_rounding"] and opt.param_groups[0]["use_stochastic_buffers"]  # the default configuration
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.cuda.manual_seed(4321)
    record = []
    for i, grs in enumerate(grads):
        for k, (p, gr) in enumerate(zip(params, grs)):
            if i == 0 and k % 7 == 3:
                p.grad = None                                     # joins at step 2: steps differ within its bucket from then on
            elif k == 1:
                p.grad = gr.t().contiguous().to(DEV).t()          # [64, 16] with strides (1, 64): step() clones it
                assert not p.grad.is_contiguous()
            else:
                p.grad = gr.clone().to(DEV)
        for key in calls:
            calls[key].clear()
        opt.step()
        torch.cuda.synchronize()
        # what the buckets of this step are: (group, dtype, quantized state) -> tensors with a gradient
        want = {}
        for p, (grp, shape, dt) in zip(params, spec):
            if p.grad is not None:
                key = (grp, dt, isinstance(opt.state[p]["exp_avg"], optim.QuantizedBuffer))
                want[key] = want.get(key, 0) + 1
        record.append(dict(offset=gen.get_offset(), buckets=want, calls={k: list(v) for k, v in calls.items()},
                           bits=[_state_bits(opt, p) for p in params], steps=[opt.state[p].get("step") for p in params]))
    return record


def test_optimizer_batches_buckets_and_keeps_every_bit(monkeypatch):
    """Three default (stochastic) steps of a two-group adapter-like model with optim.MULTI on and off: every parameter and state tensor
    bit-equal, the device generator's offset equal after every step; with MULTI on the single-tensor ops serve the buckets of one and
    each longer bucket is ONE call of a multi op, however many launches it takes."""
    from sdnq_amd import ops
    calls = {name: [] for name in ("adamw_step", "adamw_step_q8", "adamw_step_multi", "adamw_step_multi_q8")}
    for name in calls:
        def counting(*args, _fn=getattr(ops, name), _log=calls[name], _multi="multi" in name, **kw):
            _log.append(len(args[0]) if _multi else 1)
            return _fn(*args, **kw)
        monkeypatch.setattr(ops, name, counting)
    on = _run_optimizer(True, monkeypatch, calls)
    off = _run_optimizer(False, monkeypatch, calls)
    cap = capacity(False)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a["offset"] == b["offset"] and a["steps"] == b["steps"], i
        for k, (x, y) in enumerate(zip(a["bits"], b["bits"])):
            assert len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)), (i, k)
        buckets = a["buckets"]
        assert buckets == b["buckets"] and min(buckets.values()) == 1
        assert max(buckets.values()) > cap or i == 0  # from step 2 on, with every gradient there: a bucket longer than one launch
        for quantized, single, multi in ((False, "adamw_step", "adamw_step_multi"), (True, "adamw_step_q8", "adamw_step_multi_q8")):
            sizes = [n for (_, _, q), n in buckets.items() if q == quantized]
            assert sorted(a["calls"][multi]) == sorted(n for n in sizes if n > 1), (i, multi)
            assert len(a["calls"][single]) == sum(1 for n in sizes if n == 1), (i, single)
            assert b["calls"][multi] == [] and len(b["calls"][single]) == sum(sizes), (i, "MULTI off")
    assert on[0]["steps"] != on[1]["steps"] and 1 in on[1]["steps"] and 2 in on[1]["steps"]  # the late tensors lag one step


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantized", [False, True], ids=["dense", "quantized"])
def test_multi_step_is_captured_in_a_graph_and_replays_the_eager_bits(quantized):
    """tests/test_optim_gpu.py's capture test on cap + 5 tensors: two launches of the multi kernel inside the graph."""
    from sdnq_amd import optim
    n = capacity(quantized) + 5
    g = torch.Generator().manual_seed(31)
    shapes = [(32, 64) if quantized else ((16, 64), (33,), (5,))[k % 3] for k in range(n)]
    p0 = [(torch.randn(*s, generator=g) * 0.5).bfloat16() for s in shapes]
    grads = [[(torch.randn(*s, generator=g) * 0.4).bfloat16().to(DEV) for s in shapes] for _ in range(2)]
    kw = dict(lr=0.01, use_quantized_buffers=quantized, quantized_buffers_minimum_numel=512, use_stochastic_rounding=False,
              use_stochastic_buffers=False)
    eager_p, graph_p = ([torch.nn.Parameter(x.clone().to(DEV)) for x in p0] for _ in range(2))
    eager, graphed = optim.AdamW(eager_p, **kw), optim.AdamW(graph_p, **kw)
    eager.grad_scale = graphed.grad_scale = torch.tensor(2.0, device=DEV)
    for grs in grads:
        for p, gr in zip(eager_p, grs):
            p.grad = gr.clone()
        eager.step()
    for p, gr in zip(graph_p, grads[0]):
        p.grad = gr.clone()
    graphed.step()
    for p, gr in zip(graph_p, grads[1]):
        p.grad.copy_(gr)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    assert all(graphed.state[p]["step"] == 2 for p in graph_p)
    assert isinstance(graphed.state[graph_p[0]]["exp_avg"], optim.QuantizedBuffer) == quantized
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(graph_p, eager_p)):
        for x, y in zip(_state_bits(graphed, a), _state_bits(eager, b)):
            assert torch.equal(x, y), k


def test_stochastic_multi_step_still_refuses_capture():
    from sdnq_amd import optim
    params = [torch.nn.Parameter(torch.zeros(16, 64, dtype=torch.bfloat16, device=DEV)) for _ in range(3)]
    opt = optim.AdamW(params)
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    torch.cuda.synchronize()
    before = [_state_bits(opt, p) for p in params]
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    for p, old in zip(params, before):  # refused in front of every launch
        assert all(torch.equal(x, y) for x, y in zip(_state_bits(opt, p), old))
