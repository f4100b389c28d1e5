"""Host logic of the slab copy's entry points (include/sdnq_hip.h: sdnq_hip_aq_slab_bytes, sdnq_hip_aq_slab_pack,
sdnq_hip_linear_w8a8_fused_slab): sizes and argument checks, all of which return before anything is launched -- no GPU."""
from sdnq_amd import _lib

I8, BF16 = 0, 1
P = 4096  # any non-null, 16-byte aligned address


def test_slab_bytes_is_whole_32_row_blocks_of_k_bytes():
    f = _lib.load().sdnq_hip_aq_slab_bytes
    assert f(1280, 1280) == 1280 * 1280          # the SDXL projections: exactly the weight's size
    assert f(32, 128) == 32 * 128 and f(1, 128) == 32 * 128 and f(33, 128) == 64 * 128
    assert f(40, 640) == 64 * 640 and f(256, 1280) == 256 * 1280 and f(288, 1280) == 288 * 1280 and f(264, 768) == 288 * 768
    assert f(1280, 1200) == 0 and f(1280, 64) == 0  # K % 128: no copy is defined
    assert f(0, 128) == 0 and f(-32, 128) == 0 and f(32, 0) == 0 and f(32, -128) == 0


def test_slab_pack_argument_checks():
    f = _lib.load().sdnq_hip_aq_slab_pack
    assert f(None, 32, 128, 128, P, None) == -1 and f(P, 32, 128, 128, None, None) == -1  # NULL
    assert f(P, 0, 128, 128, P, None) == -3 and f(P, 32, 128, 64, P, None) == -3          # no rows; ldb < K
    assert f(P, 32, 192, 192, P, None) == -5                                              # K % 128
    assert f(P, 32, 2560, 2560, P, None) == -5                                            # K > 1280: the one-launch Linear does not take it
    assert f(P + 8, 32, 128, 128, P, None) == -4 and f(P, 32, 128, 128, P + 4, None) == -4  # misaligned source / copy
    assert f(P, 32, 128, 136, P, None) == -4                                              # a row stride that breaks the rows' alignment


def test_fused_slab_argument_checks_are_the_plain_entry_s():
    f = _lib.load().sdnq_hip_linear_w8a8_fused_slab
    assert f(I8, None, BF16, 64, 128, 128, P, P, None, 0, P, BF16, 128, P, None) == -1     # NULL activation
    assert f(2, P, BF16, 64, 128, 128, P, P, None, 0, P, BF16, 128, P, None) == -2         # unknown matmul dtype
    assert f(I8, P, BF16, 64, 128, 64, P, P, None, 0, P, BF16, 128, P, None) == -3         # ldx < K
    assert f(I8, P, BF16, 64, 192, 192, P, P, None, 0, P, BF16, 128, P, None) == -5        # K % 128
    assert f(I8, P, BF16, 64, 128, 128, P, P, None, 0, P, BF16, 128, P + 8, None) == -4    # misaligned copy
    assert f(I8, P, BF16, 64, 128, 128, None, P, None, 0, P, BF16, 128, P, None) == -1     # the copy does not replace the weight


def test_state_builds_no_slab_when_switched_off_or_without_a_cached_operand(monkeypatch):
    """linear._aq_slab answers None -- and asks the library nothing -- with SDNQ_HIP_FUSED_ROWQUANT_SLABCOPY=0, for an operand that is
    not the state's cached one (the per-call mode keeps none) and for an fp8 operand; a copy that exists is handed out as it is."""
    import torch

    from sdnq_amd import linear, ops

    def never(*a, **k):
        raise AssertionError("the library was asked for a slab copy")

    monkeypatch.setattr(ops, "aq_slab_wanted", never)
    monkeypatch.setattr(ops, "aq_slab_pack", never)
    wq = torch.zeros(256, 1280, dtype=torch.int8)
    st = linear._State()
    st.mm_weight, st.mm_slab = wq, None
    monkeypatch.setattr(linear, "FUSED_ROWQUANT_SLABCOPY", False)
    assert linear._aq_slab(st, ops.MM_I8, wq, 1024, 256, 1280) is None and st.mm_slab is None
    monkeypatch.setattr(linear, "FUSED_ROWQUANT_SLABCOPY", True)
    assert linear._aq_slab(st, ops.MM_FP8, wq, 1024, 256, 1280) is None
    assert linear._aq_slab(st, ops.MM_I8, wq.clone(), 1024, 256, 1280) is None  # not the cached operand
    st.mm_weight = None                                                         # per-call mode: row scales only
    assert linear._aq_slab(st, ops.MM_I8, wq, 1024, 256, 1280) is None and st.mm_slab is None
    st.mm_weight, st.mm_slab = wq, torch.zeros(256 * 1280, dtype=torch.int8)
    assert linear._aq_slab(st, ops.MM_I8, wq, 1024, 256, 1280) is st.mm_slab
