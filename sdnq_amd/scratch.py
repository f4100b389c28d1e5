"""The device scratch of the training side (sdnq_amd.training, sdnq_amd.lora): named uint8 buffers per device, each grown to the largest
request seen and reused by every layer.
    "operand"    the transposed weight of a backward GEMM (ops.weight_t)
    "decoded"    the second buffer a layer with SVD factors or a Hadamard rotation is dequantized into on the way there
    "unfolded"   the im2col_bwd slab of a conv backward, the float32 `cols` of its col2im route, the conv adapter's U_g
    "partials"   the float32 slab sums of ops.lowrank_grad / ops.conv_lowrank_grad
The buffers are used in stream order by the stream the backward runs on (autograd runs a node's backward on its forward's stream); a
model whose backwards run on several streams at once is not served.  (ops._workspace, the inference path's per-stream buffer, is not this.)
"""
import torch

from . import _lib

_slots: dict = {}  # (device type, device index) -> {slot name: uint8 tensor}


def _of(dev: torch.device) -> dict:
    idx = torch.cuda.current_device() if dev.index is None and dev.type == "cuda" else dev.index
    return _slots.setdefault((dev.type, idx), {})


def held(dev: torch.device) -> dict:
    """{slot name: buffer} of what `dev` holds now, as a copy: a look that allocates nothing (the byte total is the sum of its numel())."""
    return dict(_of(dev))


def take(dev: torch.device, what: str, nbytes: int, *names: str) -> list:
    """The buffers of the slots `names` on `dev`, each of at least `nbytes` bytes: one that is large enough serves as it is, a smaller or
    missing one is reallocated at `nbytes` -- not while the current stream is being captured: then `what` raises before any slot is touched."""
    slots = _of(dev)
    grow = [n for n in names if n not in slots or slots[n].numel() < nbytes]
    if grow and torch.cuda.is_current_stream_capturing():
        raise _lib.SdnqHipError(f"{what}: run one eager backward before capturing a graph (the buffer is not sized yet)")
    for n in grow:
        slots.pop(n, None)  # (the old block goes back to the allocator before the new one is taken)
        slots[n] = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    return [slots[n] for n in names]


def release() -> None:
    _slots.clear()
