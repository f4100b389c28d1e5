"""Host-side checks of the multi-tensor AdamW step that need no GPU: the capacity query, the argument checks of
sdnq_hip_adamw_step_multi / sdnq_hip_adamw_step_multi_q8 (each rule broken once, at the first, a middle and the last entry of a list
longer than one launch; every call here is refused before its first launch), the ``optim.MULTI`` switch and the routing of
``SDNQOptimizer.step`` through ``update_params_`` / ``update_param_``."""
import ctypes
import importlib.util
import sys

import pytest
import torch

from sdnq_amd import _lib, optim

NULL, DTYPE, SHAPE, ALIGN = _lib.ERR_NULL, _lib.ERR_DTYPE, _lib.ERR_SHAPE, _lib.ERR_ALIGN
SCALARS = dict(dtype=1, lr=1e-3, w1=0.1, w2=0.001, clip=1.0, decay=1.0, grad_scale=None, sr_param=0, sr_state=0, seed=0, stream=None)
DENSE_PTRS = ("params", "grads", "exp_avgs", "exp_avg_sqs")
Q8_PTRS = ("params", "grads", "m_q", "m_scale", "m_zp", "v_q", "v_scale", "v_zp")
BLOCK = 2048  # elements per workgroup


def test_capacity_needs_no_device():
    cap = _lib.load().sdnq_hip_adamw_multi_capacity
    assert 0 < cap(1) < cap(0)          # eight pointers per tensor against four
    assert cap(0) * 60 + 48 <= 4096 - 256 and cap(1) * 92 + 48 <= 4096 - 256   # the whole table is a kernel argument


class Call:
    """A valid call of one of the two entry points on `count` tensors of `numel` bf16 elements inside one 16-byte aligned host buffer,
    as columns that a test breaks one entry at a time.  It is never issued unbroken."""

    def __init__(self, q8: bool):
        lib = _lib.load()
        self.fn = lib.sdnq_hip_adamw_step_multi_q8 if q8 else lib.sdnq_hip_adamw_step_multi
        self.ptrs = Q8_PTRS if q8 else DENSE_PTRS
        self.count = 2 * lib.sdnq_hip_adamw_multi_capacity(int(q8)) + 3
        self.buf = ctypes.create_string_buffer(1 << 12)
        p = ctypes.addressof(self.buf)
        self.p = p + (-p) % 16
        self.cols = {name: [self.p] * self.count for name in self.ptrs}
        self.cols.update(numels=[64] * self.count, bc1=[0.1] * self.count, bc2=[0.001] * self.count, offsets=list(range(self.count)))

    def rc(self, count=None, drop=None, **broken):
        """The status with `drop` passed as a NULL array, column entries replaced by broken = {column: (index, value)} and scalars by
        broken = {scalar: value}."""
        n = self.count
        cols = {k: list(v) for k, v in self.cols.items()}
        scalars = dict(SCALARS)
        for key, value in broken.items():
            if key in cols:
                cols[key][value[0]] = value[1]
            else:
                scalars[key] = value
        types = dict(numels=ctypes.c_int64, bc1=ctypes.c_float, bc2=ctypes.c_float, offsets=ctypes.c_uint64)
        arrays = {k: (types.get(k, ctypes.c_void_p) * n)(*v) for k, v in cols.items()}
        if drop:
            arrays[drop] = None
        s = scalars
        return self.fn(n if count is None else count, *(arrays[k] for k in self.ptrs), arrays["numels"], arrays["bc1"], arrays["bc2"],
                       arrays["offsets"], s["dtype"], s["lr"], s["w1"], s["w2"], s["clip"], s["decay"], s["grad_scale"], s["sr_param"],
                       s["sr_state"], s["seed"], s["stream"])

    def places(self):
        return (0, self.count // 2, self.count - 1)


@pytest.mark.parametrize("q8", [False, True], ids=["dense", "q8"])
def test_entry_points_validate_every_tensor_before_any_launch(q8):
    c = Call(q8)
    assert c.count > _lib.load().sdnq_hip_adamw_multi_capacity(int(q8))
    assert c.rc(count=0) == 0 and c.rc(count=0, drop="params") == 0          # nothing to do: no launch
    assert c.rc(count=-1) == SHAPE
    for name in (*c.ptrs, "numels", "bc1", "bc2", "offsets"):                  # a NULL array
        assert c.rc(drop=name) == NULL, name
    assert c.rc(dtype=3) == DTYPE and c.rc(dtype=-1) == DTYPE
    assert c.rc(grad_scale=c.p + 2) == ALIGN
    wide = ("params", "grads", "m_q", "v_q") if q8 else DENSE_PTRS
    for at in c.places():
        for name in c.ptrs:
            assert c.rc(**{name: (at, None)}) == NULL, (name, at)              # a NULL element
            if name in wide:
                assert c.rc(**{name: (at, c.p + 8)}) == ALIGN, (name, at)      # vector access: 16 bytes
            else:
                assert c.rc(**{name: (at, c.p + 2)}) == ALIGN, (name, at)      # scale / zero point: 4 bytes
        assert c.rc(numels=(at, 0)) == SHAPE and c.rc(numels=(at, -64)) == SHAPE
        assert c.rc(numels=(at, BLOCK << 31)) == SHAPE                         # 2^31 workgroups in one launch
        if q8:
            assert c.rc(numels=(at, 48)) == SHAPE                              # not whole groups of 32
            assert c.rc(numels=(at, 32), params=(at, c.p + 8)) == ALIGN        # every tensor with uint8 state is read as vectors
        else:
            assert c.rc(numels=(at, 8), params=(at, c.p + 4)) == ALIGN         # 8 elements: the first vector access
    # two tensors of ONE launch that exceed the grid limit together, neither alone
    half = BLOCK << 30
    two = Call(q8)
    two.cols["numels"][0] = half
    assert two.rc(numels=(1, half)) == SHAPE
    last = Call(q8)
    last.cols["numels"][last.count - 2] = half
    assert last.rc(numels=(last.count - 1, half)) == SHAPE


def test_non_finite_scalars_are_refused():
    for q8 in (False, True):
        c = Call(q8)
        assert c.rc(lr=float("nan")) == _lib.ERR_UNSUPPORTED and c.rc(clip=-1.0) == _lib.ERR_UNSUPPORTED
        for at in c.places():
            assert c.rc(bc1=(at, float("inf"))) == _lib.ERR_UNSUPPORTED and c.rc(bc2=(at, float("nan"))) == _lib.ERR_UNSUPPORTED


def test_multi_follows_the_environment_variable(monkeypatch):
    """A second copy of the module under another name: the package's own module (and the identity of its classes) is left alone."""
    def fresh():
        spec = importlib.util.spec_from_file_location("sdnq_amd._optim_env_probe", optim.__file__)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.MULTI
    monkeypatch.delenv("SDNQ_HIP_OPTIM_MULTI", raising=False)
    assert fresh() is True
    for value, want in (("0", False), ("false", False), ("no", False), ("1", True)):
        monkeypatch.setenv("SDNQ_HIP_OPTIM_MULTI", value)
        assert fresh() is want, value
    assert "sdnq_amd._optim_env_probe" not in sys.modules


class OnDevice(torch.Tensor):
    """A CPU tensor that says it is on a device: step() gets past its device check and the recording hooks below launch nothing."""
    is_cuda = property(lambda self: True)


class Recorder(optim.SDNQOptimizer):
    """Knows the single-tensor hook only."""

    def __init__(self, params, **kw):
        self.single = []
        super().__init__(params, **kw)

    def init_state(self, param, group, state):
        state["exp_avg"] = torch.zeros(1)
        return state

    def update_param_(self, param, grad, group, state, grad_scale, seed, offset):
        self.single.append(param)


class BatchRecorder(Recorder):
    def __init__(self, params, **kw):
        self.batches = []
        super().__init__(params, **kw)

    def update_params_(self, group, batch, grad_scale, seed):
        self.batches.append((group, [b[0] for b in batch]))


def _fake_params():
    ps = [torch.zeros(s).as_subclass(OnDevice).requires_grad_() for s in ((4, 8), (4, 8), (4, 8), (5,), (2, 3))]
    for p in ps:
        p.grad = torch.ones(p.shape)
    return ps


def test_a_subclass_with_the_old_hook_gets_every_parameter():
    ps = _fake_params()
    opt = Recorder([dict(params=ps[:3]), dict(params=ps[3:], lr=1.0)])
    opt.step()
    assert [id(p) for p in opt.single] == [id(p) for p in ps]
    assert all(opt.state[p]["step"] == 1 for p in ps)
    # directly: the default bucket hook is the loop over the old one
    opt.single.clear()
    opt.update_params_(opt.param_groups[0], [(p, p.grad, opt.state[p], 0) for p in ps[:2]], None, 0)
    assert [id(p) for p in opt.single] == [id(p) for p in ps[:2]]


def test_buckets_and_the_switch_read_at_call_time(monkeypatch):
    ps = _fake_params()
    bf = torch.zeros(4, 8, dtype=torch.bfloat16).as_subclass(OnDevice).requires_grad_()
    bf.grad = torch.ones(4, 8, dtype=torch.bfloat16)
    off = dict(use_stochastic_rounding=False, use_stochastic_buffers=False)
    opt = BatchRecorder([dict(params=ps[:3] + [bf]), dict(params=ps[3:], lr=1.0)], **off)
    ps[1].grad = None                                       # no gradient: not in any bucket
    opt.step()
    # group 0: two float32 tensors in one bucket, the bfloat16 one alone; group 1: two float32 tensors
    assert [[id(p) for p in b[1]] for b in opt.batches] == [[id(ps[0]), id(ps[2])], [id(ps[3]), id(ps[4])]]
    assert opt.batches[0][0] is opt.param_groups[0] and opt.batches[1][0] is opt.param_groups[1]
    assert [id(p) for p in opt.single] == [id(bf)]          # a bucket of one: the single-tensor hook
    assert len(opt.state[ps[1]]) == 0 and opt.state[ps[0]]["step"] == 1
    opt.batches.clear(), opt.single.clear()
    monkeypatch.setattr(optim, "MULTI", False)              # no re-import: step() looks the switch up
    opt.step()
    assert opt.batches == [] and sorted(id(p) for p in opt.single) == sorted(id(p) for p in (ps[0], ps[2], bf, ps[3], ps[4]))


def test_cpu_parameters_raise_before_any_hook():
    p = torch.nn.Parameter(torch.zeros(4, 8))
    q = torch.nn.Parameter(torch.zeros(4, 8))
    opt = BatchRecorder([p, q])
    p.grad, q.grad = torch.ones(4, 8), torch.ones(4, 8)
    with pytest.raises(_lib.SdnqHipError, match="no CPU path"):
        opt.step()
    assert opt.single == [] and opt.batches == [] and len(opt.state[p]) == 0


def test_ops_refuse_cpu_tensors_and_mixed_lists():
    from sdnq_amd import ops
    t = [torch.zeros(64) for _ in range(2)]
    kw = dict(steps=[1, 1], offsets=[0, 1], lr=1e-3)
    with pytest.raises(_lib.SdnqHipError, match="CPU"):
        ops.adamw_step_multi(t, t, t, t, **kw)
    with pytest.raises(_lib.SdnqHipError, match="share a dtype"):
        d = [x.as_subclass(OnDevice) for x in t]
        ops.adamw_step_multi([d[0], t[1].bfloat16()], d, d, d, **kw)
    with pytest.raises(_lib.SdnqHipError, match="one entry per tensor"):
        ops.adamw_step_multi(t, t, t, t, steps=[1], offsets=[0, 1], lr=1e-3)
    ops.adamw_step_multi([], [], [], [], steps=[], offsets=[], lr=1e-3)      # nothing to do
    ops.adamw_step_multi_q8([], [], [], [], steps=[], offsets=[], lr=1e-3)
