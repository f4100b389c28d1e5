"""The scratch arena of the training side (sdnq_amd.scratch) and the workspace resolver of ops.lowrank_grad / ops.conv_lowrank_grad, host
side: the arena allocates on the device it is handed, so everything here runs on torch.device("cpu"); the capture query is patched, since
the real one needs a GPU."""
import pytest
import torch

from sdnq_amd import _lib, ops, scratch, training as T

CPU = torch.device("cpu")
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def empty_arena(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    scratch.release()
    yield
    scratch.release()


def capturing(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)


def slot(name):
    return scratch.held(CPU).get(name)


def sizes(*names):
    return tuple(None if slot(n) is None else slot(n).numel() for n in names)


def total():
    return T.scratch_bytes("cpu")


def test_a_fitting_request_is_served_and_a_larger_one_replaces_the_buffer():
    assert scratch.held(CPU) == {} and total() == 0
    (a,) = scratch.take(CPU, "x", 100, "unfolded")
    assert a.dtype == torch.uint8 and a.device == CPU and a.numel() == 100 and slot("unfolded") is a
    (b,) = scratch.take(CPU, "x", 60, "unfolded")
    assert b is a and b.numel() == 100                                   # fits: the same storage, whole
    (c,) = scratch.take(CPU, "x", 101, "unfolded")
    assert c is not a and c.numel() == 101 and slot("unfolded") is c
    (d,) = scratch.take(CPU, "x", 40, "partials")
    assert sizes("operand", "decoded", "unfolded", "partials") == (None, None, 101, 40)
    assert total() == sum(b.numel() for b in scratch.held(CPU).values()) == 141    # the sum over the slots
    assert T.scratch_bytes.__module__ == "sdnq_amd.training" and T.release_scratch.__module__ == "sdnq_amd.training"
    T.release_scratch()
    assert total() == 0 and scratch.held(CPU) == {}


@pytest.mark.parametrize("what", ("input-gradient scratch", "adapter scratch"))
def test_growing_is_refused_while_capturing_and_nothing_is_freed(what, monkeypatch):
    (a,) = scratch.take(CPU, what, 64, "partials")
    capturing(monkeypatch)
    assert scratch.take(CPU, what, 64, "partials")[0] is a and scratch.take(CPU, what, 1, "partials")[0] is a   # fits: served
    with pytest.raises(_lib.SdnqHipError) as e:
        scratch.take(CPU, what, 65, "partials")
    assert str(e.value) == f"{what}: run one eager backward before capturing a graph (the buffer is not sized yet)"
    with pytest.raises(_lib.SdnqHipError, match="before capturing"):
        scratch.take(CPU, what, 8, "operand")                            # an empty slot grows too
    assert slot("partials") is a and slot("operand") is None and total() == 64


def test_the_callers_keep_their_sentences_and_their_returns(monkeypatch):
    from sdnq_amd import lora
    assert lora._workspace(CPU, 0) is None and total() == 0
    w = lora._workspace(CPU, 48)
    assert w.dtype == torch.uint8 and w.numel() == 48 and slot("partials") is w
    u = T._scratch_unfolded(CPU, BF16, 4096)
    assert u.dtype == BF16 and u.numel() == 4096
    assert T._scratch_unfolded(CPU, BF16, 2048).numel() == 4096          # fits: the whole buffer comes back
    assert T._scratch_unfolded(CPU, torch.float32, 2048).numel() == 2048 and slot("unfolded").numel() == 8192
    capturing(monkeypatch)
    with pytest.raises(_lib.SdnqHipError, match="^adapter scratch: run one eager backward before capturing"):
        lora._workspace(CPU, 49)
    with pytest.raises(_lib.SdnqHipError, match="^input-gradient scratch: run one eager backward before capturing"):
        T._scratch_unfolded(CPU, BF16, 4097)
    assert slot("partials") is w and total() == 48 + 8192


def test_the_operand_grows_to_the_largest_and_the_decoded_buffer_follows_it():
    """training._scratch in bfloat16: "operand" grows to max(held, requested); "decoded" appears with the first two=True and from then on is
    grown with the operand, to the operand's size, whatever `two` says."""
    seen = []
    for numel, two in ((100, False), (50, False), (200, True), (80, False)):
        first, second = T._scratch(CPU, BF16, numel, two)
        assert first.dtype == BF16 and first.numel() >= numel and (second is None) == (sizes("decoded") == (None,))
        assert second is None or (second.dtype == BF16 and second.numel() == first.numel())
        seen.append(sizes("operand", "decoded"))
    assert seen == [(200, None), (200, None), (400, 400), (400, 400)]
    held = slot("operand"), slot("decoded")
    first, second = T._scratch(CPU, BF16, 80, False)                     # served: the same two storages
    assert first.data_ptr() == held[0].data_ptr() and second.data_ptr() == held[1].data_ptr()
    first, second = T._scratch(CPU, BF16, 300, False)
    assert sizes("operand", "decoded") == (600, 600) and first.numel() == second.numel() == 300
    assert total() == 1200


def test_a_refusal_over_the_decoded_buffer_leaves_the_operand_alone(monkeypatch):
    first, none = T._scratch(CPU, BF16, 100, False)
    assert none is None
    held = slot("operand")
    capturing(monkeypatch)
    assert T._scratch(CPU, BF16, 100, False)[0].data_ptr() == held.data_ptr()          # fits: served
    with pytest.raises(_lib.SdnqHipError, match="^input-gradient scratch: .*before capturing"):
        T._scratch(CPU, BF16, 100, True)                                 # the operand fits, only "decoded" would have to be made
    assert slot("operand") is held and slot("decoded") is None
    with pytest.raises(_lib.SdnqHipError, match="before capturing"):
        T._scratch(CPU, BF16, 101, True)                                 # both would grow: neither does
    assert slot("operand") is held and sizes("operand", "decoded") == (200, None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    first, second = T._scratch(CPU, BF16, 100, True)
    assert slot("operand") is held and second.numel() == 100
    capturing(monkeypatch)
    both = slot("operand"), slot("decoded")
    with pytest.raises(_lib.SdnqHipError, match="before capturing"):
        T._scratch(CPU, BF16, 101, False)
    assert slot("operand") is both[0] and slot("decoded") is both[1]
    assert T._scratch(CPU, BF16, 100, False)[1] is not None              # once present, the second buffer is handed out with the first


# ---- the workspace resolver of ops.lowrank_grad / ops.conv_lowrank_grad (ops._grad_workspace; the entry points check the device first) ----
ENTRY_POINTS = ("lowrank_grad", "conv_lowrank_grad")
NEED = 4096


@pytest.mark.parametrize("what", ENTRY_POINTS)
def test_the_resolver_names_its_entry_point_in_each_refusal(what, monkeypatch):
    assert ops._grad_workspace(what, CPU, 0, 0, None) is None            # nothing needed: nothing looked at
    with pytest.raises(_lib.SdnqHipError) as e:                          # wrong dtype
        ops._grad_workspace(what, CPU, 0, NEED, torch.empty(NEED, dtype=torch.int8))
    assert str(e.value) == f"{what}: workspace must be a uint8 device tensor of at least {NEED} bytes"
    with pytest.raises(_lib.SdnqHipError) as e:                          # too short
        ops._grad_workspace(what, CPU, 0, NEED, torch.empty(NEED - 1, dtype=torch.uint8))
    assert str(e.value) == f"{what}: workspace must be a uint8 device tensor of at least {NEED} bytes"
    base = torch.empty(NEED + 32, dtype=torch.uint8)
    off = (-base.data_ptr()) % 16                                        # base[off] lies on a 16-byte boundary
    with pytest.raises(_lib.SdnqHipError) as e:                          # exactly NEED bytes, starting one byte behind a boundary
        ops._grad_workspace(what, CPU, 0, NEED, base[off + 1:off + 1 + NEED])
    assert str(e.value) == f"{what}: workspace must hold {NEED} bytes behind its first 16-byte boundary"
    assert ops._grad_workspace(what, CPU, 0, NEED, base[off + 1:off + 16 + NEED]) == base.data_ptr() + off + 16
    assert ops._grad_workspace(what, CPU, 0, NEED, base[off:off + NEED]) == base.data_ptr() + off
    capturing(monkeypatch)                                               # the default buffer does not grow inside a capture
    monkeypatch.setattr(ops, "_workspaces", {})
    with pytest.raises(_lib.SdnqHipError) as e:
        ops._grad_workspace(what, CPU, 7, NEED, None)
    assert str(e.value) == (f"{what}: the module's workspace would have to grow inside a graph capture; pass workspace= or run one eager "
                            "call on this stream first")
    assert ops._workspaces == {}
    small = ops._workspaces[(None, 7)] = torch.empty(NEED + 15, dtype=torch.uint8)          # NEED + 16 are asked of it
    with pytest.raises(_lib.SdnqHipError, match=f"^{what}: the module's workspace would have to grow"):
        ops._grad_workspace(what, CPU, 7, NEED, None)
    assert ops._workspaces == {(None, 7): small}
    fits = ops._workspaces[(None, 7)] = torch.empty(NEED + 16, dtype=torch.uint8)
    assert ops._grad_workspace(what, CPU, 7, NEED, None) == (fits.data_ptr() + 15) & ~15 and ops._workspaces[(None, 7)] is fits


def test_the_entry_points_check_the_device_before_the_workspace():
    x = torch.zeros(16, 16, dtype=BF16)
    with pytest.raises(_lib.SdnqHipError, match="need tensors on a gfx950 device"):
        ops.lowrank_grad(x, x, workspace=torch.empty(1, dtype=torch.int8))
    with pytest.raises(_lib.SdnqHipError, match="need tensors on a gfx950 device"):
        ops.conv_lowrank_grad(x.view(1, 16, 4, 4), torch.zeros(16, 16, dtype=BF16), (1, 1), (1, 1), (0, 0), (1, 1),
                              workspace=torch.empty(1, dtype=torch.int8))
