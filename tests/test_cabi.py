"""The C-ABI shared library loads (no GPU needed) and exports every symbol include/sdnq_hip.h declares."""
import ctypes
import subprocess

import pytest

from sdnq_amd import _abi, _lib
from tests.header_util import INCLUDE, declared_arity, declared_symbols, struct_field_names


def test_library_exports_every_declared_symbol():
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 13
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/sdnq_hip.h but not exported"
    assert set(syms) == set(_lib.EXPORTS), (set(syms) ^ set(_lib.EXPORTS))


def test_version_and_strerror():
    lib = _lib.load()
    assert lib.sdnq_hip_version() == 1
    assert lib.sdnq_hip_strerror(0) == b"ok"
    for code in range(-8, 0):
        msg = lib.sdnq_hip_strerror(code)
        assert msg and msg != b"unknown status"
    assert lib.sdnq_hip_strerror(-99) == b"unknown status"


def test_argument_validation_without_gpu():
    """Validation runs before any launch, so error codes are observable on a CPU-only box."""
    lib = _lib.load()
    assert lib.sdnq_hip_rowquant(None, 1, 4, 64, 64, 0, 0, None, None, None, None, None, 0, None, None) == -1          # NULL
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    assert lib.sdnq_hip_rowquant(p, 7, 4, 64, 64, 0, 0, p, p, None, None, None, 0, None, None) == -2                  # dtype
    assert lib.sdnq_hip_rowquant(p, 1, 4, 60, 60, 0, 0, p, p, None, None, None, 0, None, None) == -3                  # K % 8
    assert lib.sdnq_hip_rowquant(p + 2, 1, 4, 64, 64, 0, 0, p, p, None, None, None, 0, None, None) == -4              # alignment
    assert lib.sdnq_hip_rowquant(p, 1, 4, 64, 64, 0, 48, p, p, None, None, None, 0, None, None) == -3                 # Hadamard group not pow2
    assert lib.sdnq_hip_scaled_mm(0, p, p, p, p, None, 0, 0, 0, p, 1, 32, 32, 24, None) == -3          # K % 16
    assert lib.sdnq_hip_scaled_mm(5, p, p, p, p, None, 0, 0, 0, p, 1, 32, 32, 32, None) == -2          # mm dtype
    w = _lib.SdnqWeight(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=16, k=64, group_size=48, svd_rank=0,
                        svd_dtype=0, storage=0, kind=0, bits=4, exponent=0, mantissa=0, native_float=0)
    assert lib.sdnq_hip_dequant(ctypes.byref(w), 0, p, 1, None) == -3                                   # K % group
    w.group_size = 64
    w.kind = 1
    assert lib.sdnq_hip_dequant(ctypes.byref(w), 0, p, 1, None) == -1                                   # uint without zero_point
    w.kind, w.bits, w.storage = 0, 9, 0
    assert lib.sdnq_hip_dequant(ctypes.byref(w), 0, p, 1, None) == -2                                   # 9 bits in uint8 words
    w.bits, w.scale_dtype = 4, 5
    assert lib.sdnq_hip_dequant(ctypes.byref(w), 0, p, 1, None) == -2                                   # unknown scale dtype
    # model-dtype-scale entry points (dequantize_fp32=False)
    assert lib.sdnq_hip_rowquant_lp(p, 0, 4, 64, 64, 0, 0, p, p, None, None, None) == -2               # float32 activations: sdnq_hip_rowquant
    assert lib.sdnq_hip_rowquant_lp(None, 1, 4, 64, 64, 0, 0, p, p, None, None, None) == -1
    assert lib.sdnq_hip_rowquant_lp(p, 1, 4, 64, 64, 1, 0, p, p, p, None, None) == -5                  # rowsum with fp8 codes
    assert lib.sdnq_hip_scaled_mm_lp(0, p, p, p, p, None, 1, 0, None, None, 0, p, 32, 32, 32, None) == -1   # bias_ndim without a bias
    assert lib.sdnq_hip_scaled_mm_lp(0, p, p, p, p, None, 0, 0, p, None, 32, p, 32, 32, 32, None) == -1     # t without svd_up
    assert lib.sdnq_hip_scaled_mm_lp(0, p, p, p, p, None, 0, 0, None, None, 0, p, 32, 32, 24, None) == -3   # K % 16
    assert lib.sdnq_hip_lowrank_down(p, 1, 4, 64, 64, p, 2, 32, p, None) == -2                         # activation / factor dtype mismatch
    assert lib.sdnq_hip_scaled_mm_lp_zp(0, p, p, p, p, None, 0, 0, None, None, 0, p, None, p, 32, 32, 32, None) == -1   # rowsum without zero point
    assert lib.sdnq_hip_scaled_mm_lp_zp(0, p, p, p, p, p, 2, 32, None, None, 0, p, p, p, 32, 32, 32, None) == -3        # zero point with a 2-D bias
    # the low-rank factors are read as 16-byte pieces: one element off (2 bytes for bf16 / f16 factors, 4 for float32) is refused, by
    # this entry as by its bf16-scale siblings
    lrk = lib.sdnq_hip_scaled_mm_lowrank
    assert lrk(0, p, p, p, p, None, 0, p + 2, p, 1, 32, None, None, None, None, p, 1, 32, 32, 32, None) == -4   # t, bf16
    assert lrk(0, p, p, p, p, None, 0, p, p + 2, 2, 32, None, None, None, None, p, 2, 32, 32, 32, None) == -4   # svd_up, f16
    assert lrk(1, p, p, p, p, None, 0, p + 4, p, 0, 32, None, None, None, None, p, 0, 32, 32, 32, None) == -4   # t, float32
    assert lrk(0, p, p, p, p, None, 0, p, p + 4, 0, 32, None, None, None, None, p, 0, 32, 32, 32, None) == -4   # svd_up, float32
    assert lrk(0, p, p, p, p, None, 0, p, None, 1, 32, None, None, None, None, p, 1, 32, 32, 32, None) == -1    # t without svd_up
    assert lib.sdnq_hip_scaled_mm_lp(0, p, p, p, p, None, 0, 0, p + 2, p, 32, p, 32, 32, 32, None) == -4
    assert lib.sdnq_hip_scaled_mm_lp_uzp_svd(p, p, p, p, None, None, None, p, p, 0, p, p + 2, 32, p, 32, 32, 32, None) == -4
    # matmuls on views (grouped convs)
    smm = lib.sdnq_hip_scaled_mm_strided
    assert smm(0, p, 16, p, p, p, None, 0, p, 32, 1, 32, 32, 32, 0, None) == -3                    # lda < K
    assert smm(0, p, 72, p, p, p, None, 0, p, 32, 1, 32, 32, 32, 0, None) == -3                    # lda % 16
    assert smm(0, p, 64, p, p, p, None, 0, p, 16, 1, 32, 32, 32, 0, None) == -3                    # ldc < N
    assert smm(0, p, 64, p, p, p, None, 0, p, 32, 1, 32, 32, 32, 12, None) == -3                   # hw % 8 / M % hw
    assert smm(0, p, 64, p, p, p, None, 0, p, 32, 0, 32, 32, 32, 16, None) == -5                   # float32 output with the NCHW store
    lfs = lib.sdnq_hip_linear_float_strided
    assert lfs(None, p, None, 1, p, 40, 32, 32, 32, 32, None) == -1
    assert lfs(p, p, None, 1, p, 40, 32, 32, 32, 16, None) == -3                                   # ldc < N
    assert lfs(p, p, None, 1, p, 40, 32, 32, 16, 32, None) == -3                                   # ldx < K


def test_weight_side_argument_validation_without_gpu():
    """The entry points on an SdnqWeight (dequant.hip, skinny.hip) validate before any launch; every value below is the status the
    library returned before these entry points were moved into units of their own."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    keep = []  # the structs, alive until the test ends (sdnq_hip_embedding takes the address as an integer)

    def weight(**kw):
        f = dict(weight=p, scale=p, zero_point=None, svd_up=None, svd_down=None, n=16, k=64, group_size=64, svd_rank=0, svd_dtype=0,
                 storage=0, kind=0, bits=4, exponent=0, mantissa=0, native_float=0)   # packed int4, one group per row
        f.update(kw)
        keep.append(_lib.SdnqWeight(**f))
        return ctypes.byref(keep[-1])

    int8 = dict(storage=2, bits=8)
    svd = dict(svd_up=p, svd_down=p, svd_rank=32, svd_dtype=1)
    sk = lib.sdnq_hip_linear_skinny
    assert sk(weight(), 0, None, None, 1, p, 1, 64, None) == -1                        # NULL x
    assert sk(weight(), 0, p, None, 7, p, 1, 64, None) == -2                           # dtype
    assert sk(weight(), 0, p, None, 1, p, 0, 64, None) == -3                           # m = 0
    assert sk(weight(), 0, p, None, 1, p, 65, 64, None) == -3                          # m > 64
    assert sk(weight(), 0, p, None, 1, p, 1, 32, None) == -3                           # ldx < K
    assert sk(weight(**svd), 0, p, None, 1, p, 1, 64, None) == -5                      # SVD factors
    assert sk(weight(), 48, p, None, 1, p, 1, 64, None) == -3                          # Hadamard group not a power of two
    assert sk(weight(), 1024, p, None, 1, p, 1, 64, None) == -3                        # Hadamard group > 512
    assert sk(weight(k=96, group_size=32), 64, p, None, 1, p, 1, 96, None) == -3       # Hadamard group does not divide K
    assert sk(weight(), 0, p + 2, None, 1, p, 1, 64, None) == -4                       # misaligned x
    ss = lib.sdnq_hip_linear_skinny_svd
    assert ss(weight(**int8, **svd), None, p, None, 1, p, 1, 64, None) == -1           # NULL svd_down_t
    assert ss(weight(**int8, **svd), p, p, None, 0, p, 1, 64, None) == -2              # float32 activations
    assert ss(weight(**int8, **svd), p, p, None, 2, p, 1, 64, None) == -2              # svd_dtype != dtype
    assert ss(weight(bits=6, **svd), p, p, None, 1, p, 1, 64, None) == -5              # packed 6-bit codes
    assert ss(weight(**int8, **svd), p, p, None, 1, p, 5, 64, None) == -3              # m > 4
    assert ss(weight(k=48, group_size=48, **int8, **svd), p, p, None, 1, p, 1, 48, None) == -3   # K % 32
    assert ss(weight(**int8, **dict(svd, svd_rank=24)), p, p, None, 1, p, 1, 64, None) == -3     # rank % 16
    assert ss(weight(**int8, **svd), p + 2, p, None, 1, p, 1, 64, None) == -4          # misaligned svd_down_t
    assert lib.sdnq_hip_requant(weight(**int8), 0, None, p, None) == -1                # NULL output
    assert lib.sdnq_hip_requant(weight(**int8), 0, p + 4, p, None) == -4               # misaligned wq
    assert lib.sdnq_hip_requant(weight(**int8), 5, p, p, None) == -2                   # mm dtype
    assert lib.sdnq_hip_requant_ws(weight(**int8), 0, None, p, 0, None) == -1
    assert lib.sdnq_hip_requant_ws(weight(**int8), 0, p + 4, p, 0, None) == -4
    assert lib.sdnq_hip_requant_ws(weight(**int8), 5, p, p, 1, None) == -2
    assert lib.sdnq_hip_requant_asym(weight(**int8), None, p, p, None) == -1
    assert lib.sdnq_hip_requant_asym(weight(**int8), p + 4, p, p, None) == -4
    assert lib.sdnq_hip_lut4_build(weight(), 0, p, 0, None, None) == -1                # NULL lut
    assert lib.sdnq_hip_lut4_build(weight(**int8), 0, p, 0, p, None) == -5             # tables exist for packed 4-bit codes only
    fp8 = dict(storage=2, kind=2, bits=8, native_float=1)
    assert lib.sdnq_hip_unpack_mm(weight(**fp8), 0, p, None) == -2                     # int8 operand from float codes
    assert lib.sdnq_hip_unpack_mm(weight(**int8), 1, p, None) == -2                    # fp8 operand from integer codes
    assert lib.sdnq_hip_unpack_mm(weight(**int8), 2, p, None) == -2                    # float16 operand from integer codes
    assert lib.sdnq_hip_unpack_mm(weight(**int8), 7, p, None) == -2                    # mm dtype
    emb = lib.sdnq_hip_embedding
    addr = lambda ref: ctypes.addressof(ref._obj)
    assert emb(addr(weight(positions=2, group_size=32)), 0, p, 1, 4, 0, 1.0, p, 1, None) == -3   # conv weight
    assert emb(addr(weight()), 0, p, 5, 4, 0, 1.0, p, 1, None) == -2                   # ids dtype
    assert emb(addr(weight()), 0, p, 1, -1, 0, 1.0, p, 1, None) == -3                  # n_ids < 0
    assert emb(addr(weight()), 48, p, 1, 4, 0, 1.0, p, 1, None) == -3                  # Hadamard group
    assert emb(addr(weight()), 0, p, 1, 0, 0, 1.0, p, 1, None) == 0                    # nothing to gather: no launch
    loss = lib.sdnq_hip_dequant_loss
    assert loss(weight(), 0, p, 1, 32, p, p, 4096, None) == -3                         # ld_ref < K
    assert loss(weight(), 0, p, 1, 64, p, p, 8, None) == -8                            # workspace of 1 partial, 4 workgroups
    assert loss(weight(), 0, p + 2, 1, 64, p, p, 4096, None) == -4                     # misaligned ref
    assert lib.sdnq_hip_dequant_loss_workspace_bytes(0, 64) == -3
    assert lib.sdnq_hip_dequant_loss_workspace_bytes(16, 64) == 32                     # one double per workgroup


def test_prefetch_argument_validation_without_gpu():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert lib.sdnq_hip_prefetch(None, 128, 0, None) == -1                       # NULL
    assert lib.sdnq_hip_prefetch(p, 0, 0, None) == 0                             # nothing to fetch: no launch
    assert lib.sdnq_hip_prefetch_hint(p, -1, None, 0, None, 0, None, 0) == -3    # negative size
    assert lib.sdnq_hip_prefetch_hint(p, 256, None, 0, p, 128, None, 0) == 0
    assert lib.sdnq_hip_prefetch_hint(None, 0, None, 0, None, 0, None, 0) == 0   # cleared again (nothing may stay pending for a later launch)


def test_attention_argument_validation_without_gpu():
    """The attention entry points validate before launching as well."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    prep = lib.sdnq_hip_attn_prepare
    ok_tail = (None, None, None, p, p, p, p, p, p, None)  # strides (contiguous), qq, qs, kq, ks, vt, kmean, stream
    assert prep(None, p, p, 1, 1, 2, 2, 8, 8, 64, 1, 0, *ok_tail) == -1                       # NULL query
    assert prep(p, p, p, 0, 1, 2, 2, 8, 8, 64, 1, 0, *ok_tail) == -5                          # float32 inputs: not built
    assert prep(p, p, p, 1, 1, 3, 2, 8, 8, 64, 1, 0, *ok_tail) == -3                          # q_heads % kv_heads
    assert prep(p, p, p, 1, 1, 2, 2, 8, 8, 136, 1, 0, *ok_tail) == -5                         # head_dim > 128
    assert prep(p, p, p, 1, 1, 2, 2, 8, 8, 60, 1, 0, *ok_tail) == -5                          # head_dim % 8
    assert prep(p, p, p, 1, 1, 2, 2, 8, 8, 64, 1, 48, *ok_tail) == -3                         # Hadamard group not a power of two
    assert prep(p + 2, p, p, 1, 1, 2, 2, 8, 8, 64, 1, 0, *ok_tail) == -4                      # alignment
    bad = (ctypes.c_int64 * 3)(1024, 516, 68)                                                 # token stride not a multiple of 8
    assert prep(p, p, p, 1, 1, 2, 2, 8, 8, 64, 1, 0, bad, None, None, p, p, p, p, p, p, None) == -4
    fwd = lib.sdnq_hip_attn_fwd
    assert fwd(p, p, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, None, 1, None, 1, 2, 2, 8, 8, 64, None) == -1    # NULL out
    assert fwd(p, p, p, p, p, 1, 0.125, 0, p, 5, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 8, 64, None) == -2          # mask dtype
    assert fwd(p, p, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 0, 64, None) == -3       # kv_len 0
    assert fwd(p, p, p, p, p, 0, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 8, 64, None) == -2       # f32 value operand
    assert fwd(None, p, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 8, 64, None) == -1    # no quantized Q
    # K / V only (qq and qs both NULL, q not read) pairs with sdnq_hip_attn_fwd_q16; one of the two alone is an error
    assert prep(p, p, p, 1, 1, 2, 2, 8, 8, 64, 1, 0, None, None, None, p, None, p, p, p, p, None) == -1
    assert prep(None, p, None, 1, 1, 2, 2, 8, 8, 64, 1, 0, None, None, None, None, None, p, p, p, p, None) == -1   # NULL value
    fq = lib.sdnq_hip_attn_fwd_q16
    assert fq(None, None, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 8, 64, None) == -1  # NULL query
    assert fq(p + 8, None, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 8, 64, None) == -4  # query rows not 16-byte aligned
    assert fq(p, bad, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 2, 2, 8, 8, 64, None) == -4       # token stride
    assert fq(p, None, p, p, p, 1, 0.125, 0, None, 0, 0, 0, 0, p, 1, None, 1, 3, 2, 8, 8, 64, None) == -3      # q_heads % kv_heads
    # the one-call form: no workspace up to 128 keys without a rotation, else the prepare pass's operands
    wsb, att = lib.sdnq_hip_attn_workspace_bytes, lib.sdnq_hip_attn
    assert wsb(1, 2, 2, 4096, 77, 64, 0) == 0 and wsb(1, 2, 2, 4096, 128, 128, 0) == 0
    assert wsb(1, 2, 2, 4096, 77, 64, 64) > 2 * 4096 * 64            # a rotation keeps the separate pass (with Q)
    assert wsb(1, 2, 1, 64, 129, 64, 0) == 160 * 64 + 768 + 160 * 64 * 2 + 32 * 64 * 4   # kq + ks (640 -> 768) + vt + channel sums, one kv head
    assert wsb(1, 3, 2, 64, 129, 64, 0) == -3 and wsb(1, 2, 2, 64, 0, 64, 0) == -3
    tail = (None, None, None, 1, 0, 0.125, 0, None, 0, 0, 0, 0)      # strides, smooth_k, hadamard_group, sm_scale, causal, mask
    assert att(p, p, None, 1, 1, 2, 2, 8, 8, 64, *tail, p, 1, None, None, 0, None) == -1       # NULL value
    assert att(p, p, p, 1, 1, 2, 2, 8, 8, 64, *tail, None, 1, None, None, 0, None) == -1       # NULL out
    assert att(p, p, p, 0, 1, 2, 2, 8, 8, 64, *tail, p, 1, None, None, 0, None) == -5          # float32 inputs
    assert att(p, p, p, 1, 1, 2, 2, 8, 200, 64, *tail, p, 1, None, None, 0, None) == -1        # > 128 keys need the workspace
    assert att(p, p, p, 1, 1, 2, 2, 8, 200, 64, *tail, p, 1, None, p, 100, None) == -3         # ... of the advertised size
    assert att(p, p + 8, p, 1, 1, 2, 2, 8, 8, 64, *tail, p, 1, None, None, 0, None) == -4      # key rows not 16-byte aligned
    # the format variants, the lse pass and the backward: every case breaks exactly ONE rule of an otherwise valid call
    def rc(fn, base, **broken):
        return fn(*{**base, **broken}.values())
    shape = dict(batch=1, qh=2, kh=2, qn=8, kn=8, d=64)
    mask = dict(mask=None, mask_dtype=0, ms_b=0, ms_h=0, ms_q=0)
    pex = lib.sdnq_hip_attn_prepare_ex
    a = dict(q=p, k=p, v=p, dtype=1, **shape, smooth=1, had=0, qst=None, kst=None, vst=None, qk=0, pv=-1, qq=p, qs=p, kq=p, ks=p, vt=p, vs=p,
             kmean=p, stream=None)
    assert rc(pex, a, q=None) == -1 and rc(pex, a, kmean=None) == -1   # NULL query; smooth_k without the channel-mean buffer
    assert rc(pex, a, qk=2) == -2                                      # Q.K^T format neither int8 nor fp8
    assert rc(pex, a, pv=7) == -2                                      # unknown P.V format
    assert rc(pex, a, pv=0, vs=None) == -1                             # quantized P.V without value scales
    assert rc(pex, a, qh=3) == -3 and rc(pex, a, kn=0) == -3
    assert rc(pex, a, d=136) == -5 and rc(pex, a, d=60) == -5
    assert rc(pex, a, had=48) == -3
    assert rc(pex, a, q=p + 2) == -4 and rc(pex, a, qst=bad) == -4
    assert rc(pex, a, dtype=0) == -5                                   # float32 inputs: not built
    fex = lib.sdnq_hip_attn_fwd_ex
    a = dict(qq=p, qs=p, kq=p, ks=p, vt=p, vs=p, v_dtype=1, qk=0, pv=-1, sm_scale=0.125, causal=0, **mask, out=p, out_dtype=1, ost=None,
             **shape, stream=None)
    assert rc(fex, a, out=None) == -1
    assert rc(fex, a, qk=2) == -2 and rc(fex, a, pv=7) == -2
    assert rc(fex, a, pv=0, vs=None) == -1
    assert rc(fex, a, qh=3) == -3 and rc(fex, a, kn=0) == -3
    assert rc(fex, a, d=136) == -5 and rc(fex, a, d=60) == -5
    assert rc(fex, a, qq=p + 2) == -4 and rc(fex, a, out=p + 2) == -4
    odd = (ctypes.c_int64 * 3)(1024, 516, 66)                          # output rows need 8 bytes only: a token stride of 68 is valid here,
    assert rc(fex, a, ost=odd) == -4                                   # one of 66 elements is not
    assert rc(fex, a, mask=p, mask_dtype=5) == -2
    assert rc(fex, a, out_dtype=5) == -2
    assert rc(fex, a, v_dtype=0) == -2                                 # f32 value operand
    lse = lib.sdnq_hip_attn_lse
    a = dict(qq=p, qs=p, kq=p, ks=p, sm_scale=0.125, causal=0, **mask, lse=p, lse_dtype=1, **shape, stream=None)
    assert rc(lse, a, qq=None) == -1 and rc(lse, a, lse=None) == -1
    assert rc(lse, a, qh=3) == -3 and rc(lse, a, kn=0) == -3
    assert rc(lse, a, d=136) == -5 and rc(lse, a, d=60) == -5
    assert rc(lse, a, qq=p + 2) == -4
    assert rc(lse, a, mask=p, mask_dtype=5) == -2
    assert rc(lse, a, lse_dtype=5) == -2
    bwd = lib.sdnq_hip_attn_bwd
    a = dict(qq=p, qs=p, kq=p, ks=p, v=p, vst=None, v_dtype=1, out=p, ost=None, grad=p, gst=None, grad_dtype=1, grad_v=p, gvst=None, lse=p,
             sm_scale=0.125, causal=0, **mask, delta=p, dq=p, dqst=None, dq_ch=64, dk=p, dkst=None, dk_ch=64, dv=p, dvst=None, **shape,
             stream=None)
    assert rc(bwd, a, kq=None) == -1 and rc(bwd, a, delta=None) == -1
    assert rc(bwd, a, qh=3) == -3 and rc(bwd, a, kn=0) == -3
    assert rc(bwd, a, d=136, dq_ch=136, dk_ch=136) == -5 and rc(bwd, a, d=60, dq_ch=60, dk_ch=60) == -5
    assert rc(bwd, a, v=p + 2) == -4 and rc(bwd, a, vst=bad) == -4
    assert rc(bwd, a, mask=p, mask_dtype=5) == -2
    assert rc(bwd, a, grad_dtype=5) == -2
    assert rc(bwd, a, v_dtype=0) == -2                                 # f32 value operand
    assert rc(bwd, a, d=40, dq_ch=48, dk_ch=40) == -3                  # dQ channels: neither head_dim nor the padded head dim


def test_bf16_uint8_matmul_argument_validation_without_gpu():
    """sdnq_hip_rowquant_lp_asym / sdnq_hip_scaled_mm_lp_uzp (the uint8 matmul on bfloat16 scales) reject bad arguments before any launch."""
    import ctypes
    from sdnq_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    rq = lib.sdnq_hip_rowquant_lp_asym
    assert rq(p, 1, 4, 64, 64, 0, p, p, None, None, None, None) == -1     # no zero-point output
    assert rq(None, 1, 4, 64, 64, 0, p, p, p, None, None, None) == -1     # NULL input
    assert rq(p, 0, 4, 64, 64, 0, p, p, p, None, None, None) == -2        # float32 rows: sdnq_hip_rowquant
    assert rq(p, 1, 4, 60, 64, 0, p, p, p, None, None, None) == -3        # K % 8
    assert rq(p, 1, 4, 64, 64, 48, p, p, p, None, None, None) == -3       # Hadamard group not a power of two
    mm = lib.sdnq_hip_scaled_mm_lp_uzp
    assert mm(p, p, p, p, None, None, None, None, p, 0, p, 4, 16, 64, None) == -1   # no activation zero points
    assert mm(p, p, p, p, None, p, None, p, p, 0, p, 4, 16, 64, None) == -1         # rowsum without a weight zero point
    assert mm(p, p, p, p, None, None, None, p, p, 0, None, 4, 16, 64, None) == -1   # NULL out
    assert mm(p, p, p, p, None, None, None, p, p, 0, p, 4, 16, 60, None) == -3      # K % 16


def test_linear_args_struct_matches_the_header():
    """The ctypes class of SdnqLinearArgs has the header's field order and the size the library checks (struct_size)."""
    assert struct_field_names("SdnqLinearArgs") == [f[0] for f in _lib.SdnqLinearArgs._fields_]
    assert ctypes.sizeof(_lib.SdnqLinearArgs) == 10 * 4 + 4 * 8 + 16 * 8


def test_one_launch_linear_predicate_and_argument_validation_without_gpu():
    """sdnq_hip_linear_w8a8_fused_supported is host logic (no launch): where the one-launch w8a8 Linear is built AND offered -- 16-bit
    activations, K % 128 == 0, K <= 1280, one round of 64 x 128 tiles, at most 12 column tiles per row block, int8 (fp8 behind its
    switch) -- and the entry point's argument checks return before anything is launched."""
    from sdnq_amd import _lib
    lib = _lib.load()
    sup = lib.sdnq_hip_linear_w8a8_fused_supported
    I8, FP8, F32, BF16, F16 = 0, 1, 0, 1, 2
    assert sup(I8, BF16, BF16, 1024, 1280, 1280) == 1 and sup(I8, F16, F16, 1024, 1280, 640) == 1
    assert sup(I8, BF16, BF16, 1024, 1280, 5120) == 0      # the rows do not fit LDS
    assert sup(I8, BF16, BF16, 1024, 1280, 1200) == 0      # K % 128
    assert sup(I8, BF16, BF16, 1024, 10240, 1280) == 0     # 80 column tiles per row block
    assert sup(I8, BF16, BF16, 2048, 1280, 1280) == 0      # 320 tiles: two rounds
    assert sup(I8, BF16, BF16, 16, 1280, 1280) == 0        # the M < 32 branch is not a matmul at all
    assert sup(I8, F32, F32, 1024, 1280, 1280) == 0 and sup(I8, BF16, F16, 1024, 1280, 1280) == 0
    assert sup(FP8, BF16, BF16, 1024, 1280, 1280) == 0     # built and bit-identical, off by default (SDNQ_HIP_FUSED_ROWQUANT_FP8)
    f = lib.sdnq_hip_linear_w8a8_fused
    p = 4096  # any non-null, 16-byte aligned address: every call below returns before a launch
    assert f(I8, None, BF16, 64, 128, 128, p, p, None, 0, p, BF16, 128, None) == -1      # NULL activation
    assert f(2, p, BF16, 64, 128, 128, p, p, None, 0, p, BF16, 128, None) == -2          # unknown matmul dtype
    assert f(I8, p, BF16, 64, 128, 64, p, p, None, 0, p, BF16, 128, None) == -3          # ldx < K
    assert f(I8, p, BF16, 64, 128, 128, p, p, None, 0, p, BF16, 132, None) == -3         # N % 8
    assert f(I8, p, BF16, 64, 192, 192, p, p, None, 0, p, BF16, 128, None) == -5         # K % 128: valid in the reference, not built here
    assert f(I8, p, BF16, 64, 2560, 2560, p, p, None, 0, p, BF16, 128, None) == -5       # K > 1280
    assert f(I8, p, F32, 64, 128, 128, p, p, None, 0, p, F32, 128, None) == -5           # float32 activations
    assert f(I8, p + 8, BF16, 64, 128, 128, p, p, None, 0, p, BF16, 128, None) == -4     # alignment


def test_scaled_mm_tile_is_a_dry_run_of_the_shape_rules():
    """sdnq_hip_scaled_mm_tile answers without a device: the tile, its threads and the workgroup count the launcher would use
    (the SDXL bs = 1 shapes of launch_tiles' comments), and refuses what sdnq_hip_scaled_mm refuses."""
    import ctypes
    lib = _lib.load()

    def tile(m, n, k, mm=0):
        bm, bn, thr, wgs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        st = lib.sdnq_hip_scaled_mm_tile(mm, 1, 1, m, n, k, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(thr), ctypes.byref(wgs))
        return st, bm.value, bn.value, thr.value, wgs.value
    assert tile(1024, 1280, 1280) == (0, 64, 128, 512, 160)      # 160 of 256 CUs: the launch the round-6 K-split tile was built against
    assert tile(1024, 10240, 1280) == (0, 256, 160, 512, 256)    # GEGLU: exactly one workgroup per CU
    assert tile(1024, 3840, 1280) == (0, 128, 128, 512, 240)
    assert tile(4608, 3072, 3072)[1:3] == (256, 256)             # FLUX: the half-tile ring
    assert tile(77, 640, 2048)[1:3] == (64, 64)
    assert tile(1024, 1280, 1280, mm=1)[0] == 0                  # fp8
    assert tile(1024, 1284, 1280)[0] != 0 and tile(0, 1280, 1280)[0] != 0 and tile(64, 64, 64, mm=7)[0] != 0
    assert lib.sdnq_hip_scaled_mm_tile(0, 1, 0, 1024, 1280, 1280, None, None, None, None) == 0  # every output pointer is optional


def test_tile_override_ids_name_their_forms_and_retired_ids_run_the_heuristics():
    """sdnq_hip_set_tile_override on int8 / bf16 / bias at 1024 x 1280 x 1280: each id launch_tiles knows reports its own form, and every
    other id -- the twenty retired ones and the first unassigned one -- reports exactly what the heuristics report, so a test that
    forces a retired id cannot pass for a form that no longer exists.  Id 28 is the K-split tile here: sdnq_internal_ks_eligible holds
    (K = 1280 is a whole number of 128-byte stages, one plain output, 32-bit tile offsets)."""
    import ctypes
    lib = _lib.load()

    def tile():
        bm, bn, thr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.sdnq_hip_scaled_mm_tile(0, 1, 1, 1024, 1280, 1280, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(thr), None) == 0
        return bm.value, bn.value, thr.value
    live = {0: (256, 256, 512), 1: (64, 128, 512), 2: (64, 64, 256), 3: (256, 128, 512), 17: (128, 128, 512), 19: (256, 128, 512),
            20: (256, 256, 512), 25: (256, 160, 512), 28: (64, 80, 512)}
    retired = [t for t in range(4, 28) if t not in live]
    assert len(retired) == 20
    try:
        lib.sdnq_hip_set_tile_override(-1)
        heuristics = tile()
        for t, form in live.items():
            lib.sdnq_hip_set_tile_override(t)
            assert tile() == form, (t, tile(), form)
        for t in retired + [29]:
            lib.sdnq_hip_set_tile_override(t)
            assert tile() == heuristics, (t, tile(), heuristics)
    finally:
        lib.sdnq_hip_set_tile_override(-1)


def test_every_export_has_declared_argument_types():
    """ctypes converts an undeclared Python int to a 32-bit C int: a device pointer or an int64 size would be truncated silently (round 6:
    a new entry point without argtypes sent truncated pointers to the GPU).  Every export must carry argtypes, as many as its prototype
    has parameters."""
    lib = _lib.load()
    raw = getattr(lib, "_ctypes", lib)
    arity = declared_arity()
    assert sorted(arity) == sorted(_lib.EXPORTS)
    wrong = [name for name in _lib.EXPORTS if getattr(raw, name).argtypes is None or len(getattr(raw, name).argtypes) != arity[name]]
    assert wrong == [], wrong


def test_the_c_compiler_accepts_everything_read_from_the_header():
    """What sdnq_amd/_abi.py read goes back to the compiler that builds csrc/binding.c, beside the header itself: every prototype in the
    reader's own spellings must be the declared type, every spelling must have the size of its ctypes type, every struct field the offset
    and size the ctypes class gives it, every enum constant its value.  A prototype, parameter or field that the reader dropped,
    reordered or misread does not compile."""
    hdr = _lib._ABI
    lines = ["#include <stddef.h>", '#include "sdnq_hip.h"']
    for ret, name, params in hdr.prototypes:
        lines.append(f'_Static_assert(__builtin_types_compatible_p(__typeof__(&{name}), {ret} (*)({", ".join(params) or "void"})), "{name}");')
        restype, argtypes = hdr.signatures[name]
        for spelling, ctype in zip([ret] + params, [restype] + argtypes):
            if ctype is not None:
                lines.append(f'_Static_assert(sizeof({spelling}) == {ctypes.sizeof(ctype)}, "{spelling} in {name}");')
    for struct, cls in hdr.classes.items():
        assert [f[0] for f in cls._fields_] == [f[0] for f in hdr.structs[struct]]
        lines.append(f'_Static_assert(sizeof({struct}) == {ctypes.sizeof(cls)}, "{struct}");')
        for field, _ in hdr.structs[struct]:
            at = getattr(cls, field)
            lines.append(f'_Static_assert(offsetof({struct}, {field}) == {at.offset} && sizeof((({struct}*)0)->{field}) == {at.size}, "{struct}.{field}");')
    lines += [f'_Static_assert({name} == {value}, "{name}");' for name, value in hdr.enums.items()]
    assert len(hdr.prototypes) == len(declared_symbols()) and len(hdr.classes) == 3 and len(hdr.enums) >= 25
    cc = subprocess.run(["gcc", "-fsyntax-only", "-Werror", "-I" + INCLUDE, "-x", "c", "-"], input="\n".join(lines) + "\n", text=True,
                        capture_output=True)
    assert cc.returncode == 0, cc.stderr


@pytest.mark.parametrize("text, line, what", [
    ("int sdnq_hip_a(int x);\nint sdnq_hip_b(long n);\n", 2, "'long'"),                        # a parameter type outside the table
    ("int sdnq_hip_a(int x);\n\nsize_t sdnq_hip_b(int x);\n", 3, "'size_t'"),                   # ... a return type
    ("int sdnq_hip_a(int x);\nint sdnq_hip_b(void (*cb)(int), int x);\n", 2, "sdnq_hip_b"),     # a declaration the prototype pattern misses
    ("int sdnq_hip_a(int x);\nint sdnq_hip_b(int x)\n{ return x; }\n", 2, "sdnq_hip_b"),
    ("int sdnq_hip_a(int);\n", 1, "not `type name`"),
    ("typedef struct S {\n    int32_t n;\n    float v[4];\n} S;\n", 3, "v[4]"),                  # an array field
    ("typedef struct S {\n    int32_t n : 3;\n} S;\n", 2, "n : 3"),                            # a bit-field
    ("typedef struct S {\n    /* c */ short n;\n} S;\n", 2, "'short'"),                        # a field type outside the table
    ("int sdnq_hip_a(const SdnqWeight* w);\n", 1, "SdnqWeight"),                               # a typed pointer whose struct was not read
    ("typedef enum E { SDNQ_A = 0, SDNQ_B } E;\n", 1, "SDNQ_B"),                               # a constant the reader would have to count
])
def test_the_header_reader_fails_closed(text, line, what):
    with pytest.raises(_abi.SdnqHipError) as e:
        _abi.Header(text)
    assert f"line {line}:" in str(e.value) and what in str(e.value), str(e.value)


def test_the_header_reader_on_a_small_header():
    hdr = _abi.Header("/* int sdnq_hip_no(int x); */\n#define N 4\ntypedef enum E { SDNQ_A = 0, SDNQ_B = -2 } E; // c\n"
                      "typedef struct SdnqWeight {\n  const void * weight;\n  int64_t m, n;\n} SdnqWeight;\n"
                      "int64_t sdnq_hip_a(const SdnqWeight *w,\n  void * const *outs, unsigned long long* id);\nvoid sdnq_hip_b(void);\n")
    assert hdr.enums == {"SDNQ_A": 0, "SDNQ_B": -2}
    assert hdr.structs == {"SdnqWeight": [("weight", "const void*"), ("m", "int64_t"), ("n", "int64_t")]}
    assert hdr.prototypes == [("int64_t", "sdnq_hip_a", ["const SdnqWeight*", "void* const*", "unsigned long long*"]), ("void", "sdnq_hip_b", [])]
    W = hdr.classes["SdnqWeight"]
    assert W._fields_ == [("weight", ctypes.c_void_p), ("m", ctypes.c_int64), ("n", ctypes.c_int64)]
    assert hdr.signatures == {"sdnq_hip_a": (ctypes.c_int64, [ctypes.POINTER(W), ctypes.c_void_p, ctypes.c_void_p]), "sdnq_hip_b": (None, [])}


def test_spot_table_of_declared_types():
    """Eight prototypes against expectations written by hand from the header; between them and the struct every row of the type table."""
    c = ctypes
    vp, i, i64, u64, f32 = c.c_void_p, c.c_int, c.c_int64, c.c_uint64, c.c_float
    want = {
        "sdnq_hip_strerror": (c.c_char_p, [i]),
        "sdnq_hip_set_tile_override": (None, [i]),
        "sdnq_hip_dequant_loss_workspace_bytes": (i64, [i64, i64]),
        "sdnq_hip_embedding": (i, [vp, i, vp, i, i64, i, c.c_double, vp, i, vp]),  # argument 0 by address, not POINTER(SdnqWeight)
        "sdnq_hip_push_post": (i, [vp, i, i, u64, u64, vp]),
        "sdnq_hip_scaled_mm_tile": (i, [i, i, i, i64, i64, i64, vp, vp, vp, vp]),
        "sdnq_hip_adamw_step": (i, [vp, vp, vp, vp, i, i64] + [f32] * 7 + [vp, i, i, u64, u64, vp]),
        "sdnq_hip_linear": (i, [c.POINTER(_lib.SdnqLinearArgs), vp]),
    }
    raw = getattr(_lib.load(), "_ctypes", _lib.load())
    for name, (restype, argtypes) in want.items():
        fn = getattr(raw, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, (name, fn.restype, fn.argtypes)
    assert _lib._ABI.signatures["sdnq_hip_embedding"][1][0] == c.POINTER(_lib.SdnqWeight) == raw.sdnq_hip_dequant.argtypes[0]
    assert _lib.SdnqWeight._fields_[4:6] == [("svd_down", vp), ("n", c.c_int32)] and list(raw.sdnq_hip_version.argtypes) == []
