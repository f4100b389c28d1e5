"""``fuse_norms(model)``: the normalisation in front of quantized Linear layers row-quantizes its own output.

In the models this package serves a LayerNorm / RMSNorm (+ the adaLN modulation) produces almost every activation a w8a8 Linear
consumes: the norm is a float kernel that writes ``y``, the layer's row quantizer a launch of its own that reads ``y`` back.
``SDNQFusedNorm`` wraps such a norm module and computes ``y`` AND its int8 / fp8 codes in one launch (``ops.norm_rowquant``,
csrc/normquant.hip), then parks the codes in the activation cache of ``linear.py`` under the key the consumers look up: every layer
that receives that very tensor object runs its GEMM on the parked codes and launches no quantizer.

Opt-in, inference only.  The fused ``y`` is the formula of ``sdnq_hip_norm_rowquant`` (float32 arithmetic, ONE rounding to the row
dtype): modules that round in between -- transformers' RMSNorm rounds before it multiplies by the weight -- differ from it in the last
bit.  Modules that merely look like an RMSNorm but compute something else (Gemma's ``x * (1 + weight)``) must not be passed.  Wrapping
moves the norm's parameters one level down (``norm1.weight`` -> ``norm1.norm.weight``): ``unfuse_norms`` before saving or loading.
"""
from __future__ import annotations

import torch

from . import linear as _L
from . import ops
from .producers import FuseResult as FuseNormsResult, fuse, hadamard_fit, unfuse


def norm_kind(mod: torch.nn.Module):
    """(ops.NORM_LAYER | ops.NORM_RMS, K) of a module the kernel can stand in for, else a sentence saying why not."""
    if isinstance(mod, SDNQFusedNorm):
        return "is fused already"
    if isinstance(mod, torch.nn.LayerNorm):
        kind, shape = ops.NORM_LAYER, tuple(mod.normalized_shape)
    else:
        # an RMSNorm by its shape (torch.nn.RMSNorm, diffusers' and transformers' classes): a [K] weight, an epsilon, no bias
        weight = getattr(mod, "weight", None)
        name = type(mod).__name__.lower()
        has_eps = any(isinstance(getattr(mod, a, None), float) for a in ("eps", "variance_epsilon")) or isinstance(mod, getattr(torch.nn, "RMSNorm", ()))
        if "rmsnorm" not in name or "gemma" in name or not isinstance(weight, torch.Tensor) or getattr(mod, "bias", None) is not None or not has_eps:
            return "is not a LayerNorm or an RMSNorm-shaped module (a [K] weight, an eps / variance_epsilon, no bias)"
        kind, shape = ops.NORM_RMS, tuple(weight.shape)
    if len(shape) != 1:
        return f"normalizes over {len(shape)} trailing dimensions (one is built)"
    if shape[0] % 8:
        return f"K = {shape[0]} is not a multiple of 8"
    return kind, shape[0]


class SDNQFusedNorm(torch.nn.Module):
    """``norm`` (an ``nn.LayerNorm`` or an RMSNorm-shaped module) computed and row-quantized in one launch; ``forward(x, scale, shift)``
    is the adaLN form ``norm(x) * (1 + scale[:, None]) + shift[:, None]`` (scale / shift: [B, K] or [B, 1, K]).

    Calls the kernel cannot serve run the wrapped module's own forward and park nothing: gradients required, CPU tensors, a dtype other
    than bf16 / f16 or than the affine parameters', inference-mode tensors (no version counter) and ``identity_reuse_disabled()``.
    When nobody used the parked codes for ``linear.UNSHARED_AFTER`` steps the kernel writes only ``y`` from then on.
    `hadamard_group` > 0: the consumers are layers quantized with ``use_hadamard`` and that ``hadamard_group_size`` -- the codes parked
    are those of the rotated row (``y`` is the same)."""

    def __init__(self, norm: torch.nn.Module, mm: str = "int8", hadamard_group: int = 0):
        super().__init__()
        kind = norm_kind(norm)
        if isinstance(kind, str):
            raise ValueError(f"SDNQFusedNorm: {type(norm).__name__} {kind}")
        misfit = hadamard_fit(hadamard_group, kind[1])
        if misfit:
            raise ValueError(f"SDNQFusedNorm: {misfit}")
        self.norm = norm
        self.kind, self.k = kind
        self.mm = ops.mm_code(mm)
        self.had = hadamard_group

    def _eps(self, dtype: torch.dtype) -> float:
        eps = getattr(self.norm, "eps", None)
        if eps is None:
            eps = getattr(self.norm, "variance_epsilon", None)
        return torch.finfo(dtype).eps if eps is None else eps  # (torch.nn.RMSNorm(eps=None))

    def _fusable(self, x: torch.Tensor, weight, bias, scale, shift) -> bool:
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() >= 1
                and x.shape[-1] == self.k and x.numel() > 0):
            return False
        if x.is_inference() or torch.is_inference_mode_enabled() or _L._ts.no_reuse:
            return False
        vectors = [t for t in (weight, bias, scale, shift) if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in [x] + vectors):
            return False
        if any(not t.is_cuda for t in vectors) or (weight is not None and weight.dtype not in (x.dtype, torch.float32)):
            return False
        if bias is not None and bias.dtype != weight.dtype:
            return False
        return scale is None or (shift is not None and scale.dtype == x.dtype and shift.dtype == x.dtype and scale.shape == shift.shape
                                 and scale.shape[-1] == self.k and (x.numel() // self.k) % (scale.numel() // self.k) == 0)

    def forward(self, x: torch.Tensor, scale: torch.Tensor | None = None, shift: torch.Tensor | None = None) -> torch.Tensor:
        norm = self.norm
        weight = getattr(norm, "weight", None)
        bias = getattr(norm, "bias", None) if self.kind == ops.NORM_LAYER else None
        if (scale is None) != (shift is None):
            raise ValueError("SDNQFusedNorm: scale and shift come together")
        if not self._fusable(x, weight, bias, scale, shift):
            y = norm(x)
            if scale is not None:  # the modulation as the models write it, over [B, rows, K]
                b = scale.numel() // self.k
                y = (y.reshape(b, -1, self.k) * (1 + scale.reshape(b, 1, self.k)) + shift.reshape(b, 1, self.k)).view(x.shape)
            return y
        x2 = x.reshape(-1, self.k)
        if x2.stride(-1) != 1 or (x2.stride(0) * x2.element_size()) % 16 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        if scale is not None:
            scale, shift = scale.reshape(-1, self.k).contiguous(), shift.reshape(-1, self.k).contiguous()
        if weight is not None:
            weight = weight.detach().contiguous()
            bias = None if bias is None else bias.detach().contiguous()
        seeding = self.__dict__.get("_sdnq_unshared", 0) < _L.UNSHARED_AFTER and _L.CACHE_ACTIVATIONS > 0
        y2, xq, xs = ops.norm_rowquant(x2, self.kind, self._eps(x.dtype), weight, bias, scale, shift, self.mm if seeding else None,
                                       hadamard_group=self.had)
        y = y2.view(x.shape)
        if xq is not None:
            _L.park_produced(y, y2, xq, xs, self.mm, self, self.had)
        return y


def _candidate(mod: torch.nn.Module) -> bool:
    """What the default walk looks at: the modules ``norm_kind`` could accept and their near misses (they get a sentence)."""
    return isinstance(mod, torch.nn.LayerNorm) or "rmsnorm" in type(mod).__name__.lower()


def fuse_norms(model: torch.nn.Module, targets=None, mm: str = "int8", hadamard_group: int = 0) -> FuseNormsResult:
    """Wrap norm modules of `model` in ``SDNQFusedNorm`` (in place).  `targets`: qualified names, or a predicate ``(name, module) -> bool``;
    by default every ``LayerNorm`` / RMSNorm-shaped module over one trailing dimension with K % 8 == 0 (a norm inside a wrapper is the
    wrapper's).  `mm`: the matmul dtype of the layers behind the norms ("int8" / "fp8") -- the parked codes serve the layers that quantize
    to it.  `hadamard_group`: the ``hadamard_group_size`` of those layers when they were quantized with ``use_hadamard`` (the parked codes
    are then those of the rotated row; a layer of another rotation quantizes for itself), 0 for un-rotated layers.  Named targets the
    kernel cannot stand in for, by default the norms it cannot, and norms whose K the group cannot rotate are listed in ``.skipped`` with
    the reason."""
    return fuse(model, targets, mm, SDNQFusedNorm, norm_kind, _candidate, hadamard_group, lambda mod, kind: kind[1])


def unfuse_norms(model: torch.nn.Module) -> int:
    """Put the wrapped norm modules back; returns how many."""
    return unfuse(model, SDNQFusedNorm, "norm")
