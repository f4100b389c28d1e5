"""What the producers of w8a8 activations share on the host: ``norms.SDNQFusedNorm`` and ``activations.SDNQFusedActivation`` wrap a
module, compute its output AND the int8 / fp8 codes of that output in one launch, and park the codes in the activation cache of
``linear.py`` for the layers that consume that very tensor (``linear.park_produced``).  Here: what ``fuse_*`` returns, the walk that
wraps a model's modules and the one that puts them back.  What a norm or an activation is, and its forward, stay in its module: a
shared forward skeleton cost 0.2-1.0 us of Python calls per forward (profiles/producer_refactor_bench.jsonl).
"""
from __future__ import annotations

import torch

from . import linear as _L
from . import ops


class FuseResult(int):
    """What ``fuse_norms()`` / ``fuse_activations()`` return: an int (the number of modules wrapped) that also carries ``.fused`` --
    their qualified names -- and ``.skipped`` -- [(qualified module name, reason)] of the candidates left as they were."""

    def __new__(cls, fused, skipped):
        r = super().__new__(cls, len(fused))
        r.fused, r.skipped = list(fused), list(skipped)
        return r

    def __iter__(self):  # `fused, skipped = fuse_norms(model)`
        return iter((self.fused, self.skipped))


def hadamard_fit(hadamard_group: int, k: int):
    """None if rows of `k` elements can be rotated in Hadamard groups of `hadamard_group` (0: no rotation), else a sentence: the rule of
    the library's ``hadamard_log2``."""
    g = hadamard_group
    if g == 0 or (isinstance(g, int) and 4 <= g <= 512 and not g & (g - 1) and k % g == 0):
        return None
    return f"hadamard_group = {g} is not a power of two in 4 .. 512 that divides the row length {k}"


def fuse(model: torch.nn.Module, targets, mm: str, wrapper, kind_of, candidate, hadamard_group: int = 0, width=None) -> FuseResult:
    """Wrap modules of `model` in `wrapper` (in place).  `targets`: qualified names, or a predicate ``(name, module) -> bool``, else
    every module `candidate(module)` accepts.  `kind_of(module)` is a sentence for a module `wrapper` cannot stand in for.  A target
    below a wrapped (or just-wrapped) module is that wrapper's and is dropped.  `hadamard_group` > 0: the wrappers park the codes of the
    rotated row; `width(module, kind)` is the row length a module's output is known to have (None: known only at its forward) and a
    module whose rows the group cannot rotate is skipped with a sentence."""
    ops.mm_code(mm)
    mods = dict(model.named_modules())
    if targets is None or callable(targets):
        names = [n for n, m in mods.items() if n and (targets(n, m) if callable(targets) else candidate(m))]
    else:
        names = list(targets)
    fused, skipped = [], []
    for name in names:
        mod = mods.get(name)
        if mod is None or not name:
            skipped.append((name, "is not a submodule of the model"))
            continue
        parents = [name[:i] for i, c in enumerate(name) if c == "."]
        if any(p in fused or isinstance(mods[p], wrapper) for p in parents):
            continue
        kind = kind_of(mod)
        if isinstance(kind, str):
            skipped.append((name, kind))
            continue
        k = width(mod, kind) if hadamard_group and width is not None else None
        misfit = hadamard_fit(hadamard_group, 0 if k is None else k)
        if misfit:
            skipped.append((name, misfit))
            continue
        parent, _, leaf = name.rpartition(".")
        setattr(mods[parent], leaf, wrapper(mod, mm, hadamard_group))
        fused.append(name)
    return FuseResult(fused, skipped)


def unfuse(model: torch.nn.Module, wrapper, attr: str) -> int:
    """Put the modules the `wrapper`s of `model` hold in `attr` back; returns how many."""
    count = 0
    for parent in list(model.modules()):
        for leaf, child in list(parent.named_children()):
            if isinstance(child, wrapper) and not isinstance(parent, wrapper):
                setattr(parent, leaf, getattr(child, attr))
                count += 1
    _L.park_seed(None)
    return count
