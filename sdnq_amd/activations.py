"""``fuse_activations(model)``: the feed-forward activation in front of a quantized Linear row-quantizes its own output.

After the norms (``fuse_norms``) the second producer of the activations a w8a8 Linear consumes is the feed-forward activation: GEGLU
in SDXL (``ff.proj_geglu`` -> ``ff.out``), GELU(tanh) in FLUX, SwiGLU in LLM blocks.  There torch runs ``chunk``, the activation and
``mul`` as two or three elementwise passes, and the layer's row quantizer reads the result once more.  ``SDNQFusedActivation`` wraps
such a module and computes the activation, the gate product, ``y`` AND its int8 / fp8 codes in one launch (``ops.act_rowquant``,
csrc/actquant.hip), then parks the codes in the activation cache of ``linear.py`` under the key the consumers look up, as
``SDNQFusedNorm`` does.

Opt-in, inference only.  The fused ``y`` is the formula of ``sdnq_hip_act_rowquant`` (float32 arithmetic, ONE rounding to the row
dtype): a module that rounds between ``gelu`` and ``mul`` differs from it in the last bit.  Wrapping moves the module's parameters one
level down (``net.0.proj.weight`` -> ``net.0.module.proj.weight``): ``unfuse_activations`` before saving or loading.
"""
from __future__ import annotations

import torch

from . import linear as _L
from . import ops
from .producers import FuseResult as FuseActivationsResult, fuse, hadamard_fit, unfuse

_PLAIN, _PROJ, _MLP = "plain", "proj", "mlp"


def _plain_act(mod):
    """The ACT_* code of an ``nn.GELU`` / ``nn.SiLU``, else a sentence."""
    if isinstance(mod, torch.nn.SiLU):
        return ops.ACT_SILU
    if isinstance(mod, torch.nn.GELU):
        approximate = getattr(mod, "approximate", "none")
        return {"none": ops.ACT_GELU, "tanh": ops.ACT_GELU_TANH}.get(approximate, f"approximates GELU by {approximate!r} (erf and tanh are built)")
    return f"is a {type(mod).__name__} (GELU, GELU(tanh) and SiLU are built)"


def _width(proj, halves: int):
    """N of the activation behind the Linear-shaped `proj` whose output holds `halves` operands side by side, else a sentence."""
    out = getattr(proj, "out_features", None)
    if not isinstance(proj, torch.nn.Module) or not isinstance(out, int):
        return "has no Linear-shaped projection (a module with out_features)"
    if out % halves or (out // halves) % 8:
        return f"N = {out} / {halves} is not a multiple of 8"
    return out // halves


def act_kind(mod: torch.nn.Module):
    """(shape, ACT_* code, gated) of a module the kernel can stand in for, else a sentence saying why not.  Shapes: "plain" (``nn.GELU``,
    ``nn.SiLU``), "proj" (a projection-owning activation: diffusers' ``GEGLU`` / ``SwiGLU`` / ``GELU``, recognised by class name and
    their ``proj``), "mlp" (``down_proj(act_fn(gate_proj(x)) * up_proj(x))``)."""
    if isinstance(mod, SDNQFusedActivation):
        return "is fused already"
    if isinstance(mod, (torch.nn.GELU, torch.nn.SiLU)):
        act = _plain_act(mod)
        return act if isinstance(act, str) else (_PLAIN, act, False)
    name = type(mod).__name__
    if all(isinstance(getattr(mod, a, None), torch.nn.Module) for a in ("gate_proj", "up_proj", "down_proj")):
        act = _plain_act(getattr(mod, "act_fn", None))
        if isinstance(act, str):
            return "its act_fn " + act
        n = _width(mod.gate_proj, 1)
        if not isinstance(n, str) and getattr(mod.up_proj, "out_features", None) != n:
            n = "gate_proj and up_proj differ in width"
        return n if isinstance(n, str) else (_MLP, act, True)
    if name in ("GEGLU", "SwiGLU", "GELU") and hasattr(mod, "proj"):
        if name == "GELU":
            act = {"none": ops.ACT_GELU, "tanh": ops.ACT_GELU_TANH}.get(getattr(mod, "approximate", None))
            if act is None:
                return f"approximates GELU by {getattr(mod, 'approximate', None)!r} (erf and tanh are built)"
        elif name == "SwiGLU":
            if not isinstance(getattr(mod, "activation", None), torch.nn.SiLU):
                return "is a SwiGLU without a SiLU `activation`"
            act = ops.ACT_SILU
        else:
            act = ops.ACT_GELU
        n = _width(mod.proj, 1 if name == "GELU" else 2)
        return n if isinstance(n, str) else (_PROJ, act, name != "GELU")
    return "is not a GELU / SiLU, a GEGLU / SwiGLU / GELU with a `proj`, or a gate_proj / up_proj / down_proj MLP"


def _out_width(mod: torch.nn.Module, kind):
    """N of the rows the module's activation writes, where its projection tells (None for a bare ``nn.GELU`` / ``nn.SiLU``)."""
    shape, _, gated = kind
    if shape == _PLAIN:
        return None
    return mod.gate_proj.out_features if shape == _MLP else mod.proj.out_features // (2 if gated else 1)


class SDNQFusedActivation(torch.nn.Module):
    """``module`` (see ``act_kind``) with its activation, gate product and the row quantization of the result in one launch.

    Calls the kernel cannot serve run the wrapped module's own forward and park nothing: gradients required, CPU tensors, a dtype other
    than bf16 / f16, a last dimension that is no multiple of 8, inference-mode tensors (no version counter) and
    ``identity_reuse_disabled()``.  When nobody used the parked codes for ``linear.UNSHARED_AFTER`` steps the kernel writes only ``y``
    from then on.  `hadamard_group` > 0: the consumers are layers quantized with ``use_hadamard`` and that ``hadamard_group_size`` --
    the codes parked are those of the rotated row (``y`` is the same); rows the group does not divide get ``y`` alone and park nothing."""

    def __init__(self, module: torch.nn.Module, mm: str = "int8", hadamard_group: int = 0):
        super().__init__()
        kind = act_kind(module)
        if isinstance(kind, str):
            raise ValueError(f"SDNQFusedActivation: {type(module).__name__} {kind}")
        misfit = hadamard_fit(hadamard_group, _out_width(module, kind) or 0)
        if misfit:
            raise ValueError(f"SDNQFusedActivation: {misfit}")
        self.module = module
        self.shape, self.act, self.gated = kind
        self.mm = ops.mm_code(mm)
        self.had = hadamard_group

    def _fusable(self, x: torch.Tensor) -> bool:
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() >= 1 and x.numel() > 0):
            return False
        if x.is_inference() or torch.is_inference_mode_enabled() or _L._ts.no_reuse:
            return False
        if self.shape == _PLAIN and x.shape[-1] % 8:
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.module.parameters())))

    @staticmethod
    def _rows(t: torch.Tensor) -> torch.Tensor:
        t2 = t.reshape(-1, t.shape[-1])
        if t2.stride(-1) != 1 or (t2.stride(0) * t2.element_size()) % 16 or t2.data_ptr() % 16:
            t2 = t2.contiguous()
        return t2

    def _launch(self, a: torch.Tensor, b: torch.Tensor | None, shape) -> torch.Tensor:
        """act(a) * b for 2-D operands -> y viewed as `shape`, its codes parked under y."""
        seeding = self.__dict__.get("_sdnq_unshared", 0) < _L.UNSHARED_AFTER and _L.CACHE_ACTIVATIONS > 0
        if self.had and a.shape[1] % self.had:
            seeding = False  # (a bare nn.GELU / nn.SiLU on rows the group does not divide: no rotated layer can consume them)
        y2, xq, xs = ops.act_rowquant(a, b, self.act, self.mm if seeding else None, hadamard_group=self.had)
        y = y2.view(shape)
        if xq is not None:
            _L.park_produced(y, y2, xq, xs, self.mm, self, self.had)
        return y

    def forward(self, x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        mod = self.module
        if not self._fusable(x):
            return mod(x, *args, **kwargs)
        if self.shape == _PLAIN:
            return self._launch(self._rows(x), None, x.shape)
        if self.shape == _MLP:
            gate, up = mod.gate_proj(x), mod.up_proj(x)
            return mod.down_proj(self._launch(self._rows(gate), self._rows(up), gate.shape))
        h = self._rows(mod.proj(x))  # diffusers' layout: [value | gate], the activation on the gate
        if not self.gated:
            return self._launch(h, None, (*x.shape[:-1], h.shape[1]))
        n = h.shape[1] // 2
        return self._launch(h[:, n:], h[:, :n], (*x.shape[:-1], n))


def _candidate(mod: torch.nn.Module) -> bool:
    """What the default walk looks at: the modules ``act_kind`` could accept and their near misses (they get a sentence)."""
    return (isinstance(mod, (torch.nn.GELU, torch.nn.SiLU)) or (type(mod).__name__ in ("GEGLU", "SwiGLU", "GELU", "ApproximateGELU") and hasattr(mod, "proj"))
            or all(hasattr(mod, a) for a in ("gate_proj", "up_proj", "down_proj")))


def fuse_activations(model: torch.nn.Module, targets=None, mm: str = "int8", hadamard_group: int = 0) -> FuseActivationsResult:
    """Wrap activation modules of `model` in ``SDNQFusedActivation`` (in place).  `targets`: qualified names, or a predicate
    ``(name, module) -> bool``; by default every module ``act_kind`` recognises, outermost first (the ``act_fn`` of a wrapped MLP is the
    wrapper's).  `mm`: the matmul dtype of the layers behind the activations ("int8" / "fp8") -- the parked codes serve the layers that
    quantize to it.  `hadamard_group`: the ``hadamard_group_size`` of those layers when they were quantized with ``use_hadamard`` (the
    parked codes are then those of the rotated row), 0 for un-rotated layers.  Named targets the kernel cannot stand in for, by default
    the near misses, and modules whose N the group cannot rotate are listed in ``.skipped`` with the reason."""
    return fuse(model, targets, mm, SDNQFusedActivation, act_kind, _candidate, hadamard_group, _out_width)


def unfuse_activations(model: torch.nn.Module) -> int:
    """Put the wrapped modules back; returns how many."""
    return unfuse(model, SDNQFusedActivation, "module")
