"""The reference's optimizer package (optim/optimizer.py, optim/adamw.py, optim/utils.py) on fused HIP launches (csrc/optim.hip):
``SDNQOptimizer`` with the reference's group keys, defaults and ``step(closure)`` contract, and ``AdamW`` on ``ops.adamw_step`` /
``ops.adamw_step_q8`` (one tensor per launch) and ``ops.adamw_step_multi`` / ``ops.adamw_step_multi_q8`` (a table of tensors per launch).

Built: parameters and gradients of float32 / bfloat16 / float16 on the device, any shape; ``lr``, ``betas``, ``weight_decay``,
``clip_threshold``, ``grad_scale``, ``final_norm_mode`` "clip" and "none"; dense state in the parameter's dtype, or -- with
``use_quantized_buffers`` for parameters of at least ``quantized_buffers_minimum_ndim`` dimensions and ``quantized_buffers_minimum_numel``
elements -- uint8 codes with a float32 scale and zero point per group of 32 along the last dimension (``QuantizedBuffer``);
``use_stochastic_rounding`` (16-bit parameters) and ``use_stochastic_buffers`` (16-bit dense state: the reference's bit trick; uint8
state: 0.1 * a standard normal added before the round).  Everything else the reference's optimizers offer raises NotImplementedError
naming the option; ``use_torch_compile`` is accepted and ignored (there is nothing to compile).

Random numbers: the kernel computes them (Philox4x32-10) from a (seed, offset) pair that ``step()`` reads from torch's device generator
once, advancing the generator's offset; parameter i of the step uses offset + i, every element its own counter.
``torch.cuda.manual_seed`` therefore reproduces a run.  Nothing here synchronises with the host.  ``state["step"]`` is a Python int,
as in the reference: a ``step()`` captured in a graph replays with the bias correction (and the random offset) of the step that was
captured, so only the deterministic configuration is captured -- a stochastic one raises while the stream is capturing.

Launches: ``step()`` collects the parameters that have a gradient into buckets keyed by (group, device, dtype, dense | quantized state)
and hands each bucket of more than one tensor to ``update_params_``, which ``AdamW`` serves with one multi-tensor call (the library
cuts it into launches of ``sdnq_hip_adamw_multi_capacity`` tensors); a bucket of one goes through ``update_param_`` and the
single-tensor entry point.  The bits of every tensor are those of its single-tensor launch either way.  Large tensors go through the
table like small ones: a set of 1482 adapter tensors and four tensors of up to 16384 x 5120 together takes the time of the two sets
apart (profiles/optim_multi_bench.jsonl, set "mixed"), and the four alone what four single-tensor launches take.  ``MULTI`` (environment
``SDNQ_HIP_OPTIM_MULTI``, default on; read at every ``step()``) set false sends every parameter through ``update_param_``: an A/B aid.
"""
from __future__ import annotations

import os
from collections.abc import Iterator

import torch

from . import _lib, ops

MULTI = os.environ.get("SDNQ_HIP_OPTIM_MULTI", "1").lower() not in {"0", "false", "no"}
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)
GROUP = 32  # elements per scale / zero point of quantized state: the reference's default quantized_buffers_group_size, the only one built
_WHOLE_TENSOR_NORMS = ("rms", "rms_clip", "relative", "rms_scaled", "rms_clip_scaled", "muon")


def _is_sdnq_tensor(t) -> bool:
    return type(t).__name__ == "SDNQTensor" or hasattr(t, "sdnq_dequantizer")


class QuantizedBuffer:
    """uint8 optimizer state: what ``SDNQTensor.from_float(x, weights_dtype="uint8", group_size=32)`` holds for a float32 tensor whose
    last dimension is a multiple of 32 -- ``weight`` uint8 [..., G, 32], ``scale`` and ``zero_point`` float32 [..., G, 1] (without the
    group axis when the last dimension is 32 itself), x ~ zero_point + weight * scale.  The kernel updates the three tensors in place."""

    def __init__(self, weight: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor, shape):
        self.weight, self.scale, self.zero_point, self.shape = weight, scale, zero_point, torch.Size(shape)

    @staticmethod
    def layout(shape):
        """(shape of the codes, shape of scale / zero point) for a tensor of `shape`."""
        k = shape[-1]
        if k % GROUP:
            raise NotImplementedError(f"quantized optimizer state needs a last dimension that is a multiple of {GROUP} (got shape "
                                      f"{tuple(shape)}): the reference's search for another group size is not built")
        if k == GROUP:
            return tuple(shape), (*shape[:-1], 1)
        return (*shape[:-1], k // GROUP, GROUP), (*shape[:-1], k // GROUP, 1)

    @classmethod
    def zeros(cls, shape, device) -> "QuantizedBuffer":
        """from_float of an all-zero tensor: scale 0, zero point 0, codes 0."""
        ws, ss = cls.layout(shape)
        return cls(torch.zeros(ws, dtype=torch.uint8, device=device), torch.zeros(ss, dtype=torch.float32, device=device),
                   torch.zeros(ss, dtype=torch.float32, device=device), shape)

    @property
    def device(self):
        return self.weight.device

    def parts(self):
        return self.weight, self.scale, self.zero_point

    def dequantize(self, dtype: torch.dtype | None = None) -> torch.Tensor:
        out = torch.addcmul(self.zero_point, self.weight.to(torch.float32), self.scale).view(self.shape)
        return out if dtype is None else out.to(dtype)

    def to(self, device) -> "QuantizedBuffer":
        """A copy on `device`."""
        return QuantizedBuffer(*(t.to(device, copy=True) for t in self.parts()), self.shape)

    def clone(self) -> "QuantizedBuffer":
        return self.to(self.device)

    def __repr__(self) -> str:
        return f"QuantizedBuffer(shape={tuple(self.shape)}, device={self.device})"


torch.serialization.add_safe_globals([QuantizedBuffer])


class SDNQOptimizer(torch.optim.Optimizer):
    """SDNQOptimizer (optim/optimizer.py:13-144): group keys and defaults, ``step(closure)`` with ``state["step"]``, lazy
    ``init_state`` and ``self.grad_scale``.  A subclass gives ``init_state`` and ``update_param_``, the one fused launch of one tensor,
    and may give ``update_params_``, the launch of a whole bucket."""

    _base_group_keys = frozenset({
        "params", "lr", "betas", "weight_decay", "clip_threshold", "final_norm_mode", "use_kahan", "use_cautious", "use_torch_compile",
        "use_stochastic_rounding", "use_stochastic_buffers", "use_quantized_buffers", "quantized_buffers_dtype",
        "quantized_buffers_minimum_numel", "quantized_buffers_minimum_ndim", "quantized_buffers_hadamard_group_size",
        "quantized_buffers_svd_rank", "quantized_buffers_svd_steps", "quantized_buffers_codebook_steps", "quantized_buffers_group_size",
        "quantized_buffers_use_svd", "quantized_buffers_use_hadamard", "quantized_buffers_use_codebook", "offload_buffers",
        "offload_non_blocking", "offload_non_blocking_cpu",
    })
    _extra_group_keys = frozenset()
    _group_keys = _base_group_keys | _extra_group_keys
    _step_supports_amp_scaling = True
    # (key, default) in the reference's order (optim/optimizer.py:52-78); offload_non_blocking_cpu defaults to offload_non_blocking
    _DEFAULTS = (
        ("lr", 1e-4), ("betas", (0.9, 0.999)), ("weight_decay", 0.01), ("clip_threshold", (1.0, 1e-3, 1e-3)), ("final_norm_mode", "clip"),
        ("use_kahan", False), ("use_cautious", False), ("use_torch_compile", False), ("use_stochastic_rounding", True),
        ("use_stochastic_buffers", True), ("use_quantized_buffers", False), ("quantized_buffers_dtype", "uint8"),
        ("quantized_buffers_minimum_numel", 16384), ("quantized_buffers_minimum_ndim", 2), ("quantized_buffers_hadamard_group_size", 256),
        ("quantized_buffers_svd_rank", 32), ("quantized_buffers_svd_steps", 8), ("quantized_buffers_codebook_steps", 24),
        ("quantized_buffers_group_size", 32), ("quantized_buffers_use_svd", False), ("quantized_buffers_use_hadamard", False),
        ("quantized_buffers_use_codebook", False), ("offload_buffers", False), ("offload_non_blocking", True),
    )

    @staticmethod
    def get_default_kwarg(group: dict, kwargs: dict, key: str, default):
        return group.get(key, kwargs.get(key, default))

    @staticmethod
    def apply_group_defaults(group: dict, **kwargs) -> dict:
        for key, default in SDNQOptimizer._DEFAULTS:
            group[key] = SDNQOptimizer.get_default_kwarg(group, kwargs, key, default)
        group["offload_non_blocking_cpu"] = SDNQOptimizer.get_default_kwarg(group, kwargs, "offload_non_blocking_cpu", group["offload_non_blocking"])
        return group

    def __init__(self, params, **kwargs):
        # the reference's forms (optim/adamw.py:17-26) -- a parameter, an iterator of them, a list of them, or a list of group dicts --
        # and, as torch.optim takes them, plain tensors where the reference insists on nn.Parameter
        if isinstance(params, (torch.Tensor, Iterator)) or (isinstance(params, (list, tuple)) and len(params) > 0 and isinstance(params[0], torch.Tensor)):
            kwargs["params"] = params
            param_groups = [kwargs]
        else:
            param_groups = params
        for group in param_groups:
            self.apply_group_defaults(group, **kwargs)
            unknown = set(group.keys()) - self._group_keys
            if unknown:
                raise ValueError(f"{type(self).__name__}: unknown option(s) {sorted(unknown)}")
            self.check_group(group)
        super().__init__(param_groups, {})
        for group in self.param_groups:
            for param in group["params"]:
                self.check_param(param, group)

    # ---- what is built ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def check_group(cls, group: dict) -> None:
        """Raise NotImplementedError naming the first option of `group` that is not built."""
        name = cls.__name__
        for key in ("use_kahan", "use_cautious", "offload_buffers"):
            if group[key]:
                raise NotImplementedError(f"{name}: {key} is not built")
        mode = group["final_norm_mode"]
        if mode not in ("clip", "none"):
            why = "it needs a norm over the whole tensor" if mode in _WHOLE_TENSOR_NORMS else "the reference does not know it either"
            raise NotImplementedError(f"{name}: final_norm_mode={mode!r} is not built ({why}); built: 'clip', 'none'")
        if group["use_quantized_buffers"]:
            for key in ("quantized_buffers_use_svd", "quantized_buffers_use_hadamard", "quantized_buffers_use_codebook"):
                if group[key]:
                    raise NotImplementedError(f"{name}: {key} is not built")
            if group["quantized_buffers_dtype"] != "uint8":
                raise NotImplementedError(f"{name}: quantized_buffers_dtype={group['quantized_buffers_dtype']!r} is not built (built: 'uint8')")
            if group["quantized_buffers_group_size"] != GROUP:
                raise NotImplementedError(f"{name}: quantized_buffers_group_size={group['quantized_buffers_group_size']} is not built (built: {GROUP})")

    @staticmethod
    def quantizes(param: torch.Tensor, group: dict) -> bool:
        """The reference's rule for which parameters get quantized state (optim/adamw.py:30)."""
        return bool(group["use_quantized_buffers"] and param.ndim >= group["quantized_buffers_minimum_ndim"]
                    and param.numel() >= group["quantized_buffers_minimum_numel"])

    @classmethod
    def check_param(cls, param: torch.Tensor, group: dict) -> None:
        if _is_sdnq_tensor(param):
            raise NotImplementedError(f"{cls.__name__}: SDNQTensor parameters (quantized weights) are not built; pass float parameters")
        if param.dtype not in _FLOATS:
            raise NotImplementedError(f"{cls.__name__}: parameters of float32 / bfloat16 / float16 are built (got {param.dtype})")
        if cls.quantizes(param, group):
            QuantizedBuffer.layout(param.shape)

    # ---- the subclass's part ------------------------------------------------------------------------------------------------------------
    def init_state(self, param: torch.Tensor, group: dict, state: dict) -> dict:
        raise NotImplementedError

    def update_param_(self, param: torch.Tensor, grad: torch.Tensor, group: dict, state: dict, grad_scale, seed: int, offset: int) -> None:
        raise NotImplementedError

    def update_params_(self, group: dict, batch: list, grad_scale, seed: int) -> None:
        """Update every (param, grad, state, offset) of `batch`: tensors of one group, device, dtype and state form.  Here: one by one."""
        for param, grad, state, offset in batch:
            self.update_param_(param, grad, group, state, grad_scale, seed, offset)

    @staticmethod
    def needs_random(param: torch.Tensor, group: dict) -> bool:
        if param.dtype != torch.float32 and (group["use_stochastic_rounding"] or group["use_stochastic_buffers"]):
            return True
        return bool(group["use_stochastic_buffers"] and SDNQOptimizer.quantizes(param, group))

    # ---- step -----------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        grad_scale = getattr(self, "grad_scale", None)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        scales = {}   # device -> grad_scale as one float32 there
        drawn = {}    # device -> [generator, seed, first offset, tensors served]
        buckets = {}  # (group index, device, dtype, quantized state, seed) -> (group, [(param, grad, state, offset)], grad_scale, seed)
        for index, group in enumerate(self.param_groups):
            self.check_group(group)
            for param in group["params"]:
                if param.grad is None:
                    continue
                self.check_param(param, group)
                if not param.is_cuda:
                    raise _lib.SdnqHipError(f"{type(self).__name__}.step needs its parameters on a gfx950 device (got a CPU tensor); "
                                            "there is no CPU path")
                grad = param.grad
                if grad.is_sparse or grad.dtype != param.dtype:
                    raise NotImplementedError(f"{type(self).__name__}: dense gradients of the parameter's dtype are built "
                                              f"(got {'sparse ' if grad.is_sparse else ''}{grad.dtype} for {param.dtype})")
                if not param.is_contiguous() or param.data_ptr() % 16:
                    raise NotImplementedError(f"{type(self).__name__}: contiguous, 16-byte aligned parameters are built")
                if not grad.is_contiguous() or grad.data_ptr() % 16:
                    grad = grad.clone(memory_format=torch.contiguous_format)
                state = self.state[param]
                if len(state) == 0:
                    state["step"] = 0
                    state = self.init_state(param, group, state)
                state["step"] += 1
                dev = param.device
                gs = None
                if grad_scale is not None:
                    if dev not in scales:
                        t = grad_scale if isinstance(grad_scale, torch.Tensor) else torch.tensor(float(grad_scale))
                        scales[dev] = t.detach().to(device=dev, dtype=torch.float32, non_blocking=True).reshape(-1)[:1].contiguous()
                    gs = scales[dev]
                seed = offset = 0
                if self.needs_random(param, group):
                    if dev not in drawn:
                        if torch.cuda.is_current_stream_capturing():
                            raise RuntimeError(f"{type(self).__name__}.step: stochastic rounding draws its (seed, offset) on the host and "
                                               "cannot be captured in a graph; capture with use_stochastic_rounding=False and "
                                               "use_stochastic_buffers=False")
                        gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
                        drawn[dev] = [gen, gen.initial_seed(), gen.get_offset(), 0]
                    d = drawn[dev]
                    seed, offset = d[1], d[2] + d[3]
                    d[3] += 1
                quantized = any(isinstance(value, QuantizedBuffer) for value in state.values())
                bucket = buckets.setdefault((index, dev, param.dtype, quantized, seed), (group, [], gs, seed))
                bucket[1].append((param, grad, state, offset))
        multi = MULTI
        for group, batch, gs, seed in buckets.values():
            if multi and len(batch) > 1:
                self.update_params_(group, batch, gs, seed)
            else:
                for param, grad, state, offset in batch:
                    self.update_param_(param, grad, group, state, gs, seed, offset)
        for gen, _seed, first, used in drawn.values():
            gen.set_offset(first + (used + 3) // 4 * 4)  # torch keeps the offset a multiple of 4
        return loss

    # ---- state dict -------------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: dict) -> None:
        """torch's load_state_dict (dense state is cast to the parameter's dtype and device, "step" is kept), then every
        QuantizedBuffer, which torch passes through by reference, becomes this optimizer's own copy on its parameter's device."""
        super().load_state_dict(state_dict)
        for param, state in self.state.items():
            for key, value in state.items():
                if isinstance(value, QuantizedBuffer):
                    state[key] = value.to(param.device if isinstance(param, torch.Tensor) else value.device)
                elif key == "step" and isinstance(value, torch.Tensor):
                    state[key] = int(value.item())


class AdamW(SDNQOptimizer):
    """AdamW (optim/adamw.py:12-50): state keys ``step``, ``exp_avg``, ``exp_avg_sq``; the whole update of a parameter, or of a bucket
    of them, is one launch."""

    def init_state(self, param: torch.Tensor, group: dict, state: dict) -> dict:
        if self.quantizes(param, group):
            state["exp_avg"] = QuantizedBuffer.zeros(param.shape, param.device)
            state["exp_avg_sq"] = QuantizedBuffer.zeros(param.shape, param.device)
        else:
            state["exp_avg"] = torch.zeros_like(param, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.contiguous_format)
        return state

    @staticmethod
    def _options(group: dict, grad_scale, seed: int) -> dict:
        clips = group["clip_threshold"]
        return dict(lr=group["lr"], betas=group["betas"], weight_decay=group["weight_decay"],
                    clip=clips if isinstance(clips, (int, float)) else clips[0], grad_scale=grad_scale,
                    sr_param=group["use_stochastic_rounding"], sr_state=group["use_stochastic_buffers"], seed=seed)

    @staticmethod
    def _moments(state: dict):
        """(exp_avg, exp_avg_sq, quantized) with quantized state as its (codes, scale, zero point) triples."""
        m, v = state["exp_avg"], state["exp_avg_sq"]
        if isinstance(m, QuantizedBuffer) != isinstance(v, QuantizedBuffer):
            raise ValueError("AdamW: exp_avg and exp_avg_sq must both be dense or both be quantized")
        return (m.parts(), v.parts(), True) if isinstance(m, QuantizedBuffer) else (m, v, False)

    def update_param_(self, param, grad, group, state, grad_scale, seed, offset) -> None:
        m, v, quantized = self._moments(state)
        (ops.adamw_step_q8 if quantized else ops.adamw_step)(param, grad, m, v, step=state["step"], offset=offset,
                                                             **self._options(group, grad_scale, seed))

    def update_params_(self, group, batch, grad_scale, seed) -> None:
        if type(self).update_param_ is not AdamW.update_param_:  # a subclass that changed the single-tensor hook keeps it
            return super().update_params_(group, batch, grad_scale, seed)
        moments = [self._moments(state) for _, _, state, _ in batch]
        if any(m[2] != moments[0][2] for m in moments):
            raise ValueError("AdamW: the tensors of one bucket must all have dense or all have quantized state")
        (ops.adamw_step_multi_q8 if moments[0][2] else ops.adamw_step_multi)(
            [b[0] for b in batch], [b[1] for b in batch], [m[0] for m in moments], [m[1] for m in moments],
            steps=[b[2]["step"] for b in batch], offsets=[b[3] for b in batch], **self._options(group, grad_scale, seed))


def _not_built(name: str, what: str):
    class _NotBuilt:
        def __init__(self, *args, **kwargs):
            raise NotImplementedError(f"{name}: {what} is not built (AdamW is: sdnq_amd.optim.AdamW)")
    _NotBuilt.__name__ = _NotBuilt.__qualname__ = name
    return _NotBuilt


# the reference's other optimizers, importable by name: a caller that reaches one learns what is missing
NOT_BUILT = {
    "Adafactor": "the factored second-moment optimizer (optim/adafactor.py)",
    "CAME": "the confidence-guided optimizer (optim/came.py)",
    "Lion": "the sign-momentum optimizer (optim/lion.py)",
    "Muon": "the Newton-Schulz orthogonalizing optimizer (optim/muon.py)",
}
globals().update({name: _not_built(name, what) for name, what in NOT_BUILT.items()})

__all__ = ["SDNQOptimizer", "AdamW", "QuantizedBuffer", *NOT_BUILT]
