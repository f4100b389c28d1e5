// Fused AdamW step for gfx950: one launch per parameter tensor, or per table of small ones, one pass over the parameter, everything in
// float32 registers.
//
// Reference chain replaced (about 25 elementwise torch passes per parameter there, plus a dequantize and a re-quantize of two buffers
// when the state is quantized; ONE launch here):
//   grad  = clamp(nan_to_num_(g).float() / grad_scale, -clip, clip) ; p32 = nan_to_num_(p).float()        optim/utils.py:26-43
//   m     = lerp_(m, grad, 1 - beta1) ; v = lerp_(v, grad^2, 1 - beta2)   (+ storing both)                 optim/utils.py:120-135, adamw.py:65-69
//   u     = clamp(nan_to_num(m / (1 - beta1^t) * rsqrt(v / (1 - beta2^t))), -clip, clip)                   optim/adamw.py:66-73
//   u     = norm mode "none" / "clip": nan_to_num and the same clamp again -- both leave u as it is          optim/utils.py:139-151
//   p32   = p32 * (1 - lr * wd)   (wd != 0) ; p32 = p32 + (-lr) * u ; p = round(p32)                        optim/utils.py:66-67, 86-89
//   16-bit storage with stochastic rounding: copy_stochastic_                                               optim/utils.py:113-116
//   uint8 state: SDNQTensor.dequantize (addcmul(zp, q, scale), dequantizer.py) and SDNQTensor.copy_ -> from_float -> quantize_weight
//   (min / max per group of 32, scale = (max - min) / 255, q = round((m - min) / scale), + 0.1 * randn before the round when
//   stochastic)                                                                                             quant_utils.py:10-19, 28-56
//
// Order of the float32 operations: the reference's, operation by operation.  Contraction: the unit is compiled with -ffp-contract=off,
// so a multiply and an add are ONE rounding only where the source says fmaf -- and it says so exactly where torch's own kernels fuse:
//   lerp_          fmaf(w, b - a, a) for w < 0.5, fmaf(w - 1, b - a, b) otherwise   (ATen lerp: vec::fmadd on the CPU, contracted on a device)
//   add_(u, alpha) fmaf(u, -lr, p)                                                  (ATen add with alpha: the same)
//   addcmul        fmaf(q, scale, zp)                                               (the dequantization of uint8 state)
// Everything else rounds after every operation: g / grad_scale, m / bc1 and v / bc2 are IEEE divisions (torch on the CPU divides; on a
// device it multiplies by the float reciprocal of the scalar, one ulp away at most), g * g, p * decay and m_hat * rsqrt(v_hat) are plain
// products.  rsqrt is the device's (v_rsq_f32 with denormal scaling, 1 ulp), where the CPU computes 1 / sqrt: it reaches the parameter
// scaled by lr and none of the state.
//
// Layout: a lane owns 8 consecutive elements (one 16-byte load / store per 16-bit tensor, two per float32 tensor), a block 2048.
// uint8 state: a group of 32 is four adjacent lanes of one wave (numel % 32 == 0, so a group never straddles a wave or the end); its
// min and max meet by two DPP quad exchanges, no LDS, no atomics; the lane with (lane & 3) == 0 stores the group's scale and zero
// point, every lane its 8 codes as one 8-byte store.
// Tail: a lane whose 8 elements lie past the end re-reads element 0 and stores nothing (colquant.hip's masking); the one lane that
// holds the last numel % 8 elements of a dense tensor loads and stores them one by one.
// Random numbers: Philox4x32-10, key = seed, counter = (element index / 8, stream << 28 in the high word, offset): the bits an element
// gets depend on (seed, offset, element index) alone, not on the launch geometry.  Streams: 0 parameter, 1 exp_avg, 2 exp_avg_sq
// (16-bit stochastic rounding: one call serves 8 elements, 16 bits each); 1, 3 and 2, 4: the two calls behind the 8 Box-Muller normals
// of a stochastic uint8 buffer.
// NaN: fminf / fmaxf drop a NaN operand, so the clamps here turn a NaN into a bound where torch's clamp keeps it; every clamp of the
// chain follows a nan_to_num, so none sees one.  A group whose min equals its max gets scale 0 and codes 0 (0 / 0 cast to uint8 in the
// reference, see quant_pack_kernel in quantize.hip).
//
// Many tensors in one launch (adamw_dense_multi_kernel, adamw_q8_multi_kernel): a block is still 2048 consecutive elements of ONE
// tensor, the grid is the tensors' block ranges one after the other.  The table of tensors -- per tensor its pointers, numel, bc1, bc2
// and Philox offset, and in a column of its own the tensor's first block -- travels BY VALUE in the kernel arguments beside the shared
// scalars: no device-side table, no workspace, no copy, so the call is captured like the single-tensor one.  blockIdx.x is uniform, so
// the binary search over the first-block column and the reads of the record are scalar loads from the argument segment.  A block then
// fills an AdamWScalars and runs the single-tensor chain with indices relative to its tensor's start: the bits of
// sdnq_hip_adamw_step(_q8) on that tensor alone, random bits included (they depend on seed, offset and the element index only).
// Capacity: HIP documents 4096 bytes of kernel arguments.  hipcc enforces nothing (a 64 KB by-value argument compiles without a
// diagnostic), so the bound is a static_assert here, and it leaves room for the whole argument segment: 4096 less the 256 bytes of implicit
// arguments the compiler appends to a kernel that uses them (these do not) = 3840.  The shared scalars take 48, a tensor 56 + 4 (dense: four pointers) or 88 + 4 (uint8 state:
// eight), which gives (3840 - 48) / 60 = 63 and (3840 - 48) / 92 = 41 tensors per launch.  The entry points cut a longer list into
// launches.
#include "philox_dev.h"  // aw_philox: shared with the dropout of the adapter kernels

namespace {

constexpr int AW_BLOCK = 256;
constexpr int AW_EPL = 8;  // elements per lane

struct AdamWScalars {
    float neg_lr, w1, w2, bc1, bc2, clip, decay;
    const float* grad_scale;  // device, one float32, or NULL
    u32 seed_lo, seed_hi, off_lo, off_hi;
    int sr_param, sr_state;
};

template <int T_ID> struct AwLimits;
template <> struct AwLimits<SDNQ_F32> { static constexpr float max = 3.4028234663852886e38f; };
template <> struct AwLimits<SDNQ_BF16> { static constexpr float max = 3.3895313892515355e38f; static constexpr u32 step = 0x10000u; };
template <> struct AwLimits<SDNQ_F16> { static constexpr float max = 65504.0f; static constexpr u32 step = 0x2000u; };

// torch.nan_to_num of a value held in dtype T_ID: nan -> 0, +-inf -> the dtype's largest finite value
template <int T_ID>
__device__ __forceinline__ float aw_nan_to_num(float x) {
    if (x != x) return 0.0f;
    if (x == __builtin_inff()) return AwLimits<T_ID>::max;
    if (x == -__builtin_inff()) return -AwLimits<T_ID>::max;
    return x;
}
__device__ __forceinline__ float aw_clamp(float x, float c) { return fminf(fmaxf(x, -c), c); }

// ATen's lerp with a scalar weight
__device__ __forceinline__ float aw_lerp(float a, float b, float w) {
    const float diff = b - a;
    return (w < 0.5f) ? fmaf(w, diff, a) : fmaf(w - 1.0f, diff, b);
}

__device__ __forceinline__ uint4 aw_random(const AdamWScalars& a, int64_t e8, u32 stream) {
    return aw_philox((u32)e8, (u32)((uint64_t)e8 >> 32) | (stream << 28), a.off_lo, a.off_hi, a.seed_lo, a.seed_hi);
}

// copy_stochastic_ (optim/utils.py:113-116): add a uniform integer below 2^(23 - mantissa) to the float32 bits, mask, clamp; the
// conversion to the 16-bit dtype that follows is exact (bf16) or rounds only float16 subnormals
template <int T_ID>
__device__ __forceinline__ float aw_sr(float x, u32 r16) {
    if constexpr (T_ID == SDNQ_F32) {
        return x;
    } else {
        constexpr u32 step = AwLimits<T_ID>::step;
        const float y = __uint_as_float((__float_as_uint(x) + (r16 & (step - 1u))) & ~(step - 1u));
        return (y != y) ? y : aw_clamp(y, AwLimits<T_ID>::max);
    }
}
// 8 values -> their storage rounding, in place: round-to-nearest-even happens in the store; the stochastic form rounds here
template <int T_ID>
__device__ __forceinline__ void aw_sr8(float (&v)[8], const AdamWScalars& a, int64_t e8, u32 stream) {
    const uint4 r = aw_random(a, e8, stream);
    const u32 w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = aw_sr<T_ID>(v[e], (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));
}

// 8 consecutive elements at element index idx: `nv` of them exist (8: vector access; 1..7: the tail lane, one by one)
template <int T_ID>
__device__ __forceinline__ void aw_load8(const void* base, int64_t idx, int nv, float (&v)[8]) {
    if (nv == AW_EPL) {
        if constexpr (T_ID == SDNQ_F32) {
            Vec16<SDNQ_F32>::unpack(*(const uint4*)((const float*)base + idx), v);
            Vec16<SDNQ_F32>::unpack(*(const uint4*)((const float*)base + idx + 4), v + 4);
        } else {
            Vec16<T_ID>::unpack(*(const uint4*)((const uint16_t*)base + idx), v);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (e < nv) ? FT<T_ID>::load(base, idx + e) : 0.0f;
    }
}
template <int T_ID>
__device__ __forceinline__ void aw_store8(void* base, int64_t idx, int nv, const float (&v)[8]) {
    if (nv == AW_EPL) {
        if constexpr (T_ID == SDNQ_F32) {
            *(uint4*)((float*)base + idx) = Vec16<SDNQ_F32>::pack(v);
            *(uint4*)((float*)base + idx + 4) = Vec16<SDNQ_F32>::pack(v + 4);
        } else {
            *(uint4*)((uint16_t*)base + idx) = Vec16<T_ID>::pack(v);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e < nv) FT<T_ID>::store(base, idx + e, v[e]);
        }
    }
}

// steps 1-7 of the chain for one element: p, m, v hold the old values on entry and the new float32 values on return
template <int T_ID>
__device__ __forceinline__ void aw_update(float& p, float g, float& m, float& v, const AdamWScalars& a, float gs, bool has_gs) {
    g = aw_nan_to_num<T_ID>(g);
    if (has_gs) g = g / gs;
    g = aw_clamp(g, a.clip);
    p = aw_nan_to_num<T_ID>(p);
    m = aw_lerp(m, g, a.w1);
    v = aw_lerp(v, g * g, a.w2);
    const float m_hat = m / a.bc1;
    const float v_hat = v / a.bc2;
    float u = m_hat * rsqrtf(v_hat);
    u = aw_clamp(aw_nan_to_num<SDNQ_F32>(u), a.clip);  // the norm modes "none" and "clip" change nothing after this
    p = p * a.decay;                                   // decay = 1 when weight_decay == 0: exact
    p = fmaf(u, a.neg_lr, p);
}

// ---- dense state: exp_avg / exp_avg_sq in the parameter's dtype ----------------------------------------------------------------------
template <int T_ID>
__global__ __launch_bounds__(AW_BLOCK) void adamw_dense_kernel(void* __restrict__ param, const void* __restrict__ grad,
                                                               void* __restrict__ exp_avg, void* __restrict__ exp_avg_sq, int64_t numel,
                                                               const AdamWScalars a) {
    const int64_t e8 = (int64_t)blockIdx.x * AW_BLOCK + threadIdx.x;
    const int64_t left = numel - e8 * AW_EPL;
    const int nv = left >= AW_EPL ? AW_EPL : (left > 0 ? (int)left : 0);
    // a masked lane re-reads the start of the tensor: 8 elements, or all of a tensor shorter than that
    const int nl = nv ? nv : (numel >= AW_EPL ? AW_EPL : (int)numel);
    const int64_t idx = nv ? e8 * AW_EPL : 0;
    float p[8], g[8], m[8], v[8];
    aw_load8<T_ID>(param, idx, nl, p);
    aw_load8<T_ID>(grad, idx, nl, g);
    aw_load8<T_ID>(exp_avg, idx, nl, m);
    aw_load8<T_ID>(exp_avg_sq, idx, nl, v);
    const bool has_gs = a.grad_scale != nullptr;
    const float gs = has_gs ? *a.grad_scale : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) aw_update<T_ID>(p[e], g[e], m[e], v[e], a, gs, has_gs);
    if constexpr (T_ID != SDNQ_F32) {
        if (a.sr_param) aw_sr8<T_ID>(p, a, e8, 0u);
        if (a.sr_state) {
            aw_sr8<T_ID>(m, a, e8, 1u);
            aw_sr8<T_ID>(v, a, e8, 2u);
        }
    }
    if (nv == 0) return;
    aw_store8<T_ID>(param, idx, nv, p);
    aw_store8<T_ID>(exp_avg, idx, nv, m);
    aw_store8<T_ID>(exp_avg_sq, idx, nv, v);
}

// ---- uint8 state: codes [numel], scale and zero point [numel / 32] float32 -----------------------------------------------------------
__device__ __forceinline__ float aw_quad_min(float x) {
    x = fminf(x, __int_as_float(lane_xor_i32(__float_as_int(x), 1)));
    return fminf(x, __int_as_float(lane_xor_i32(__float_as_int(x), 2)));
}
__device__ __forceinline__ float aw_quad_max(float x) {
    x = fmaxf(x, __int_as_float(lane_xor_i32(__float_as_int(x), 1)));
    return fmaxf(x, __int_as_float(lane_xor_i32(__float_as_int(x), 2)));
}
__device__ __forceinline__ void aw_dequant8(const uint2 c, float scale, float zp, float (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = fmaf((float)(((e < 4 ? c.x : c.y) >> (8 * (e & 3))) & 0xffu), scale, zp);
}
// 8 standard normals from two Philox calls (Box-Muller on 24-bit uniforms: |n| <= sqrt(2 * 24 * ln 2) = 5.77)
__device__ __forceinline__ void aw_normal8(const AdamWScalars& a, int64_t e8, u32 s0, u32 s1, float (&n)[8]) {
    const uint4 r0 = aw_random(a, e8, s0), r1 = aw_random(a, e8, s1);
    const u32 w[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float u1 = (float)((w[2 * i] >> 8) + 1u) * 5.9604644775390625e-8f;  // (0, 1]
        const float u2 = (float)(w[2 * i + 1] >> 8) * 5.9604644775390625e-8f;     // [0, 1): the angle in revolutions
        const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // sqrt(-2 ln u1), logf = log2
        n[2 * i] = rad * __builtin_amdgcn_cosf(u2);
        n[2 * i + 1] = rad * __builtin_amdgcn_sinf(u2);
    }
}
// quantize_weight (quant_utils.py:28-56) of the lane's 8 values with its group's three neighbours: scale, zero point and 8 codes
__device__ __forceinline__ uint2 aw_quant8(const float (&x)[8], bool stochastic, const AdamWScalars& a, int64_t e8, u32 s0, u32 s1,
                                           float& scale, float& zp) {
    float lo = x[0], hi = x[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) { lo = fminf(lo, x[e]); hi = fmaxf(hi, x[e]); }
    lo = aw_quad_min(lo);
    hi = aw_quad_max(hi);
    scale = (hi - lo) / 255.0f;
    zp = lo;
    RowDiv rd;
    rd.set(scale);
    float q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float d = x[e] - lo;
        q[e] = rd.fast ? rd.fastdiv(d) : d / scale;  // the correctly rounded quotient either way (RowDiv, sdnq_dev.h)
    }
    if (stochastic) {
        float n[8];
        aw_normal8(a, e8, s0, s1, n);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = q[e] + 0.1f * n[e];  // add_(randn, alpha=0.1): alpha * randn rounds, then the add
    }
    u32 c[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float r = __builtin_rintf(q[e]);
        r = (r != r) ? 0.0f : fminf(fmaxf(r, 0.0f), 255.0f);
        c[e >> 2] |= (u32)r << (8 * (e & 3));
    }
    return make_uint2(c[0], c[1]);
}

template <int T_ID>
__global__ __launch_bounds__(AW_BLOCK) void adamw_q8_kernel(void* __restrict__ param, const void* __restrict__ grad, int64_t numel,
                                                            uint8_t* __restrict__ m_q, float* __restrict__ m_scale, float* __restrict__ m_zp,
                                                            uint8_t* __restrict__ v_q, float* __restrict__ v_scale, float* __restrict__ v_zp,
                                                            const AdamWScalars a) {
    const int64_t e8 = (int64_t)blockIdx.x * AW_BLOCK + threadIdx.x;
    const bool ok = e8 * AW_EPL < numel;  // numel % 32 == 0: all four lanes of a group agree
    const int64_t idx = ok ? e8 * AW_EPL : 0;
    const int64_t grp = idx >> 5;
    float p[8], g[8], m[8], v[8];
    aw_load8<T_ID>(param, idx, AW_EPL, p);
    aw_load8<T_ID>(grad, idx, AW_EPL, g);
    const uint2 mc = *(const uint2*)(m_q + idx), vc = *(const uint2*)(v_q + idx);
    aw_dequant8(mc, m_scale[grp], m_zp[grp], m);
    aw_dequant8(vc, v_scale[grp], v_zp[grp], v);
    const bool has_gs = a.grad_scale != nullptr;
    const float gs = has_gs ? *a.grad_scale : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) aw_update<T_ID>(p[e], g[e], m[e], v[e], a, gs, has_gs);
    if constexpr (T_ID != SDNQ_F32) {
        if (a.sr_param) aw_sr8<T_ID>(p, a, e8, 0u);
    }
    float ms, mz, vs, vz;
    const uint2 mn = aw_quant8(m, a.sr_state != 0, a, e8, 1u, 3u, ms, mz);
    const uint2 vn = aw_quant8(v, a.sr_state != 0, a, e8, 2u, 4u, vs, vz);
    if (!ok) return;
    aw_store8<T_ID>(param, idx, AW_EPL, p);
    *(uint2*)(m_q + idx) = mn;
    *(uint2*)(v_q + idx) = vn;
    if ((threadIdx.x & 3) == 0) {
        m_scale[grp] = ms; m_zp[grp] = mz;
        v_scale[grp] = vs; v_zp[grp] = vz;
    }
}

// ---- many tensors in one launch ------------------------------------------------------------------------------------------------------
struct AwShared {
    float neg_lr, w1, w2, clip, decay;
    int count;                // tensors in this launch, 1 .. capacity
    const float* grad_scale;  // device, one float32, or NULL
    u32 seed_lo, seed_hi;
    int sr_param, sr_state;
};
struct AwDenseRec {
    void* param; const void* grad; void* exp_avg; void* exp_avg_sq;
    int64_t numel;
    uint64_t offset;
    float bc1, bc2;
};
struct AwQ8Rec {
    void* param; const void* grad;
    uint8_t* m_q; float* m_scale; float* m_zp;
    uint8_t* v_q; float* v_scale; float* v_zp;
    int64_t numel;
    uint64_t offset;
    float bc1, bc2;
};
constexpr int AW_KERNARG_BYTES = 4096 - 256;  // the documented 4 KB less 256 bytes of implicit arguments
template <class Rec>
struct AwTable {
    static constexpr int CAP = (AW_KERNARG_BYTES - (int)sizeof(AwShared)) / (int)(sizeof(Rec) + sizeof(u32));
    AwShared s;
    Rec rec[CAP];
    u32 first[CAP];  // the tensor's first block: ascending, first[0] == 0
};
static_assert(sizeof(AwTable<AwDenseRec>) <= AW_KERNARG_BYTES && AwTable<AwDenseRec>::CAP == 63, "dense table: 63 tensors");
static_assert(sizeof(AwTable<AwQ8Rec>) <= AW_KERNARG_BYTES && AwTable<AwQ8Rec>::CAP == 41, "uint8-state table: 41 tensors");

// the tensor that block `b` belongs to: the last i with first[i] <= b.  Uniform over the block: scalar loads, at most 6 rounds
template <class Rec>
__device__ __forceinline__ int aw_find(const AwTable<Rec>& t, u32 b) {
    int lo = 0, hi = t.s.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}
template <class Rec>
__device__ __forceinline__ AdamWScalars aw_scalars_of(const AwShared& s, const Rec& r) {
    AdamWScalars a;
    a.neg_lr = s.neg_lr; a.w1 = s.w1; a.w2 = s.w2; a.bc1 = r.bc1; a.bc2 = r.bc2; a.clip = s.clip; a.decay = s.decay;
    a.grad_scale = s.grad_scale;
    a.seed_lo = s.seed_lo; a.seed_hi = s.seed_hi; a.off_lo = (u32)r.offset; a.off_hi = (u32)(r.offset >> 32);
    a.sr_param = s.sr_param; a.sr_state = s.sr_state;
    return a;
}

// adamw_dense_kernel's chain on the block's own tensor; e8 counts from the tensor's first block
template <int T_ID>
__global__ __launch_bounds__(AW_BLOCK) void adamw_dense_multi_kernel(const AwTable<AwDenseRec> t) {
    const int i = aw_find(t, blockIdx.x);
    const AwDenseRec& r = t.rec[i];
    const AdamWScalars a = aw_scalars_of(t.s, r);
    void* const param = r.param; const void* const grad = r.grad; void* const exp_avg = r.exp_avg; void* const exp_avg_sq = r.exp_avg_sq;
    const int64_t numel = r.numel;
    const int64_t e8 = (int64_t)(blockIdx.x - t.first[i]) * AW_BLOCK + threadIdx.x;
    const int64_t left = numel - e8 * AW_EPL;
    const int nv = left >= AW_EPL ? AW_EPL : (left > 0 ? (int)left : 0);
    const int nl = nv ? nv : (numel >= AW_EPL ? AW_EPL : (int)numel);
    const int64_t idx = nv ? e8 * AW_EPL : 0;
    float p[8], g[8], m[8], v[8];
    aw_load8<T_ID>(param, idx, nl, p);
    aw_load8<T_ID>(grad, idx, nl, g);
    aw_load8<T_ID>(exp_avg, idx, nl, m);
    aw_load8<T_ID>(exp_avg_sq, idx, nl, v);
    const bool has_gs = a.grad_scale != nullptr;
    const float gs = has_gs ? *a.grad_scale : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) aw_update<T_ID>(p[e], g[e], m[e], v[e], a, gs, has_gs);
    if constexpr (T_ID != SDNQ_F32) {
        if (a.sr_param) aw_sr8<T_ID>(p, a, e8, 0u);
        if (a.sr_state) {
            aw_sr8<T_ID>(m, a, e8, 1u);
            aw_sr8<T_ID>(v, a, e8, 2u);
        }
    }
    if (nv == 0) return;
    aw_store8<T_ID>(param, idx, nv, p);
    aw_store8<T_ID>(exp_avg, idx, nv, m);
    aw_store8<T_ID>(exp_avg_sq, idx, nv, v);
}

// adamw_q8_kernel's chain on the block's own tensor: numel % 32 == 0 per tensor and a block never spans two, so a group of four lanes
// is whole here as well
template <int T_ID>
__global__ __launch_bounds__(AW_BLOCK) void adamw_q8_multi_kernel(const AwTable<AwQ8Rec> t) {
    const int i = aw_find(t, blockIdx.x);
    const AwQ8Rec& r = t.rec[i];
    const AdamWScalars a = aw_scalars_of(t.s, r);
    void* const param = r.param; const void* const grad = r.grad;
    uint8_t* const m_q = r.m_q; float* const m_scale = r.m_scale; float* const m_zp = r.m_zp;
    uint8_t* const v_q = r.v_q; float* const v_scale = r.v_scale; float* const v_zp = r.v_zp;
    const int64_t e8 = (int64_t)(blockIdx.x - t.first[i]) * AW_BLOCK + threadIdx.x;
    const bool ok = e8 * AW_EPL < r.numel;
    const int64_t idx = ok ? e8 * AW_EPL : 0;
    const int64_t grp = idx >> 5;
    float p[8], g[8], m[8], v[8];
    aw_load8<T_ID>(param, idx, AW_EPL, p);
    aw_load8<T_ID>(grad, idx, AW_EPL, g);
    const uint2 mc = *(const uint2*)(m_q + idx), vc = *(const uint2*)(v_q + idx);
    aw_dequant8(mc, m_scale[grp], m_zp[grp], m);
    aw_dequant8(vc, v_scale[grp], v_zp[grp], v);
    const bool has_gs = a.grad_scale != nullptr;
    const float gs = has_gs ? *a.grad_scale : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) aw_update<T_ID>(p[e], g[e], m[e], v[e], a, gs, has_gs);
    if constexpr (T_ID != SDNQ_F32) {
        if (a.sr_param) aw_sr8<T_ID>(p, a, e8, 0u);
    }
    float ms, mz, vs, vz;
    const uint2 mn = aw_quant8(m, a.sr_state != 0, a, e8, 1u, 3u, ms, mz);
    const uint2 vn = aw_quant8(v, a.sr_state != 0, a, e8, 2u, 4u, vs, vz);
    if (!ok) return;
    aw_store8<T_ID>(param, idx, AW_EPL, p);
    *(uint2*)(m_q + idx) = mn;
    *(uint2*)(v_q + idx) = vn;
    if ((threadIdx.x & 3) == 0) {
        m_scale[grp] = ms; m_zp[grp] = mz;
        v_scale[grp] = vs; v_zp[grp] = vz;
    }
}

int aw_scalars(AdamWScalars& a, float lr, float w1, float w2, float bc1, float bc2, float clip, float decay, const float* grad_scale,
               int sr_param, int sr_state, uint64_t seed, uint64_t offset) {
    // finite scalars only: a NaN here would reach every element
    const float f[7] = {lr, w1, w2, bc1, bc2, clip, decay};
    for (float x : f) {
        if (!(x == x) || x == __builtin_inff() || x == -__builtin_inff()) return SDNQ_ERR_UNSUPPORTED;
    }
    if (w1 < 0.0f || w1 > 1.0f || w2 < 0.0f || w2 > 1.0f || clip < 0.0f) return SDNQ_ERR_UNSUPPORTED;
    a.neg_lr = -lr; a.w1 = w1; a.w2 = w2; a.bc1 = bc1; a.bc2 = bc2; a.clip = clip; a.decay = decay;
    a.grad_scale = grad_scale;
    a.seed_lo = (u32)seed; a.seed_hi = (u32)(seed >> 32); a.off_lo = (u32)offset; a.off_hi = (u32)(offset >> 32);
    a.sr_param = sr_param ? 1 : 0; a.sr_state = sr_state ? 1 : 0;
    return SDNQ_OK;
}

}  // namespace

extern "C" int sdnq_hip_adamw_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int dtype, int64_t numel, float lr,
                                   float w1, float w2, float bc1, float bc2, float clip, float decay, const float* grad_scale,
                                   int sr_param, int sr_state, uint64_t seed, uint64_t offset, sdnq_stream_t stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    if (numel <= 0) return SDNQ_ERR_SHAPE;
    // vector access needs 16-byte alignment; a tensor shorter than 8 elements is all tail and is read element by element
    if (numel >= AW_EPL && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16)) return SDNQ_ERR_ALIGN;
    if (grad_scale && ((uintptr_t)grad_scale % 4)) return SDNQ_ERR_ALIGN;
    AdamWScalars a;
    const int st = aw_scalars(a, lr, w1, w2, bc1, bc2, clip, decay, grad_scale, sr_param, sr_state, seed, offset);
    if (st != SDNQ_OK) return st;
    const int64_t blocks = (numel + AW_BLOCK * AW_EPL - 1) / (AW_BLOCK * AW_EPL);
    if (blocks > 0x7fffffff) return SDNQ_ERR_SHAPE;
    const dim3 grid((unsigned)blocks), block(AW_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case SDNQ_F32: hipLaunchKernelGGL((adamw_dense_kernel<SDNQ_F32>), grid, block, 0, s, param, grad, exp_avg, exp_avg_sq, numel, a); break;
        case SDNQ_BF16: hipLaunchKernelGGL((adamw_dense_kernel<SDNQ_BF16>), grid, block, 0, s, param, grad, exp_avg, exp_avg_sq, numel, a); break;
        default: hipLaunchKernelGGL((adamw_dense_kernel<SDNQ_F16>), grid, block, 0, s, param, grad, exp_avg, exp_avg_sq, numel, a); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_adamw_step_q8(void* param, const void* grad, int dtype, int64_t numel, void* exp_avg_q, float* exp_avg_scale,
                                      float* exp_avg_zp, void* exp_avg_sq_q, float* exp_avg_sq_scale, float* exp_avg_sq_zp, float lr,
                                      float w1, float w2, float bc1, float bc2, float clip, float decay, const float* grad_scale,
                                      int sr_param, int sr_state, uint64_t seed, uint64_t offset, sdnq_stream_t stream) {
    if (!param || !grad || !exp_avg_q || !exp_avg_scale || !exp_avg_zp || !exp_avg_sq_q || !exp_avg_sq_scale || !exp_avg_sq_zp) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    if (numel <= 0 || (numel % 32) != 0) return SDNQ_ERR_SHAPE;
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg_q | (uintptr_t)exp_avg_sq_q) % 16)) return SDNQ_ERR_ALIGN;
    if ((((uintptr_t)exp_avg_scale | (uintptr_t)exp_avg_zp | (uintptr_t)exp_avg_sq_scale | (uintptr_t)exp_avg_sq_zp | (uintptr_t)grad_scale) % 4)) return SDNQ_ERR_ALIGN;
    AdamWScalars a;
    const int st = aw_scalars(a, lr, w1, w2, bc1, bc2, clip, decay, grad_scale, sr_param, sr_state, seed, offset);
    if (st != SDNQ_OK) return st;
    const int64_t blocks = (numel + AW_BLOCK * AW_EPL - 1) / (AW_BLOCK * AW_EPL);
    if (blocks > 0x7fffffff) return SDNQ_ERR_SHAPE;
    const dim3 grid((unsigned)blocks), block(AW_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define AW_Q8_LAUNCH(T)                                                                                                              \
    hipLaunchKernelGGL((adamw_q8_kernel<T>), grid, block, 0, s, param, grad, numel, (uint8_t*)exp_avg_q, exp_avg_scale, exp_avg_zp, \
                       (uint8_t*)exp_avg_sq_q, exp_avg_sq_scale, exp_avg_sq_zp, a)
    switch (dtype) {
        case SDNQ_F32: AW_Q8_LAUNCH(SDNQ_F32); break;
        case SDNQ_BF16: AW_Q8_LAUNCH(SDNQ_BF16); break;
        default: AW_Q8_LAUNCH(SDNQ_F16); break;
    }
#undef AW_Q8_LAUNCH
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

// ---- many tensors in one launch: entry points ----------------------------------------------------------------------------------------
namespace {

constexpr int64_t AW_PER_BLOCK = AW_BLOCK * AW_EPL;
constexpr int64_t AW_GRID_MAX = 0x7fffffff;

int aw_shared(AwShared& s, float lr, float w1, float w2, float clip, float decay, const float* grad_scale, int sr_param, int sr_state,
              uint64_t seed) {
    AdamWScalars a;
    const int st = aw_scalars(a, lr, w1, w2, 1.0f, 1.0f, clip, decay, grad_scale, sr_param, sr_state, seed, 0);
    if (st != SDNQ_OK) return st;
    s.neg_lr = a.neg_lr; s.w1 = a.w1; s.w2 = a.w2; s.clip = a.clip; s.decay = a.decay; s.count = 0;
    s.grad_scale = grad_scale; s.seed_lo = a.seed_lo; s.seed_hi = a.seed_hi; s.sr_param = a.sr_param; s.sr_state = a.sr_state;
    return SDNQ_OK;
}
bool aw_finite(float x) { return x == x && x != __builtin_inff() && x != -__builtin_inff(); }

// the checks that do not depend on the state's form, for all `count` tensors, and the grid of every launch of `cap` tensors
int aw_multi_check(int64_t count, int cap, const void* const* const* arrays, int n_arrays, const int64_t* numels, const float* bc1,
                   const float* bc2, const uint64_t* offsets, int dtype, const float* grad_scale, bool q8) {
    if (count < 0) return SDNQ_ERR_SHAPE;
    if (count == 0) return SDNQ_OK;
    for (int k = 0; k < n_arrays; ++k) {
        if (!arrays[k]) return SDNQ_ERR_NULL;
    }
    if (!numels || !bc1 || !bc2 || !offsets) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    if (grad_scale && ((uintptr_t)grad_scale % 4)) return SDNQ_ERR_ALIGN;
    int64_t blocks = 0;
    for (int64_t i = 0; i < count; ++i) {
        uintptr_t wide = 0, narrow = 0;  // addresses that need 16 bytes / 4 bytes
        for (int k = 0; k < n_arrays; ++k) {
            const void* ptr = arrays[k][i];
            if (!ptr) return SDNQ_ERR_NULL;
            // uint8 state: param, grad and the two code arrays (0, 1, 2, 5) are read as vectors, scale and zero point as floats
            ((q8 && k != 0 && k != 1 && k != 2 && k != 5) ? narrow : wide) |= (uintptr_t)ptr;
        }
        const int64_t n = numels[i];
        if (n <= 0 || (q8 && (n % 32) != 0)) return SDNQ_ERR_SHAPE;
        if ((q8 || n >= AW_EPL) && (wide % 16)) return SDNQ_ERR_ALIGN;
        if (narrow % 4) return SDNQ_ERR_ALIGN;
        if (!aw_finite(bc1[i]) || !aw_finite(bc2[i])) return SDNQ_ERR_UNSUPPORTED;
        if (i % cap == 0) blocks = 0;
        blocks += (n - 1) / AW_PER_BLOCK + 1;
        if (blocks > AW_GRID_MAX) return SDNQ_ERR_SHAPE;
    }
    return SDNQ_OK;
}

template <class Rec, class Fill, class Launch>
int aw_multi_launch(int64_t count, const int64_t* numels, const float* bc1, const float* bc2, const uint64_t* offsets, AwTable<Rec>& t,
                    Fill fill, Launch launch) {
    constexpr int cap = AwTable<Rec>::CAP;
    for (int64_t base = 0; base < count; base += cap) {
        const int n = (int)(count - base < cap ? count - base : cap);
        u32 blocks = 0;
        for (int j = 0; j < n; ++j) {
            const int64_t i = base + j;
            fill(t.rec[j], i);
            t.rec[j].numel = numels[i]; t.rec[j].offset = offsets[i]; t.rec[j].bc1 = bc1[i]; t.rec[j].bc2 = bc2[i];
            t.first[j] = blocks;
            blocks += (u32)((numels[i] - 1) / AW_PER_BLOCK + 1);
        }
        t.s.count = n;
        launch(dim3(blocks), t);
        SDNQ_CHECK_LAUNCH();
    }
    return SDNQ_OK;
}

}  // namespace

extern "C" int sdnq_hip_adamw_multi_capacity(int quantized) { return quantized ? AwTable<AwQ8Rec>::CAP : AwTable<AwDenseRec>::CAP; }

extern "C" int sdnq_hip_adamw_step_multi(int64_t count, void* const* params, const void* const* grads, void* const* exp_avgs,
                                         void* const* exp_avg_sqs, const int64_t* numels, const float* bc1, const float* bc2,
                                         const uint64_t* offsets, int dtype, float lr, float w1, float w2, float clip, float decay,
                                         const float* grad_scale, int sr_param, int sr_state, uint64_t seed, sdnq_stream_t stream) {
    using Table = AwTable<AwDenseRec>;
    const void* const* const arrays[4] = {(const void* const*)params, grads, (const void* const*)exp_avgs, (const void* const*)exp_avg_sqs};
    int st = aw_multi_check(count, Table::CAP, arrays, 4, numels, bc1, bc2, offsets, dtype, grad_scale, false);
    if (st != SDNQ_OK || count == 0) return st;
    Table t{};
    st = aw_shared(t.s, lr, w1, w2, clip, decay, grad_scale, sr_param, sr_state, seed);
    if (st != SDNQ_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    return aw_multi_launch(count, numels, bc1, bc2, offsets, t,
        [&](AwDenseRec& r, int64_t i) { r.param = params[i]; r.grad = grads[i]; r.exp_avg = exp_avgs[i]; r.exp_avg_sq = exp_avg_sqs[i]; },
        [&](dim3 grid, const Table& tab) {
            switch (dtype) {
                case SDNQ_F32: hipLaunchKernelGGL((adamw_dense_multi_kernel<SDNQ_F32>), grid, dim3(AW_BLOCK), 0, s, tab); break;
                case SDNQ_BF16: hipLaunchKernelGGL((adamw_dense_multi_kernel<SDNQ_BF16>), grid, dim3(AW_BLOCK), 0, s, tab); break;
                default: hipLaunchKernelGGL((adamw_dense_multi_kernel<SDNQ_F16>), grid, dim3(AW_BLOCK), 0, s, tab); break;
            }
        });
}

extern "C" int sdnq_hip_adamw_step_multi_q8(int64_t count, void* const* params, const void* const* grads, void* const* exp_avg_qs,
                                            void* const* exp_avg_scales, void* const* exp_avg_zps, void* const* exp_avg_sq_qs,
                                            void* const* exp_avg_sq_scales, void* const* exp_avg_sq_zps, const int64_t* numels,
                                            const float* bc1, const float* bc2, const uint64_t* offsets, int dtype, float lr, float w1,
                                            float w2, float clip, float decay, const float* grad_scale, int sr_param, int sr_state,
                                            uint64_t seed, sdnq_stream_t stream) {
    using Table = AwTable<AwQ8Rec>;
    const void* const* const arrays[8] = {(const void* const*)params, grads, (const void* const*)exp_avg_qs,
                                          (const void* const*)exp_avg_scales, (const void* const*)exp_avg_zps,
                                          (const void* const*)exp_avg_sq_qs, (const void* const*)exp_avg_sq_scales,
                                          (const void* const*)exp_avg_sq_zps};
    int st = aw_multi_check(count, Table::CAP, arrays, 8, numels, bc1, bc2, offsets, dtype, grad_scale, true);
    if (st != SDNQ_OK || count == 0) return st;
    Table t{};
    st = aw_shared(t.s, lr, w1, w2, clip, decay, grad_scale, sr_param, sr_state, seed);
    if (st != SDNQ_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    return aw_multi_launch(count, numels, bc1, bc2, offsets, t,
        [&](AwQ8Rec& r, int64_t i) {
            r.param = params[i]; r.grad = grads[i];
            r.m_q = (uint8_t*)exp_avg_qs[i]; r.m_scale = (float*)exp_avg_scales[i]; r.m_zp = (float*)exp_avg_zps[i];
            r.v_q = (uint8_t*)exp_avg_sq_qs[i]; r.v_scale = (float*)exp_avg_sq_scales[i]; r.v_zp = (float*)exp_avg_sq_zps[i];
        },
        [&](dim3 grid, const Table& tab) {
            switch (dtype) {
                case SDNQ_F32: hipLaunchKernelGGL((adamw_q8_multi_kernel<SDNQ_F32>), grid, dim3(AW_BLOCK), 0, s, tab); break;
                case SDNQ_BF16: hipLaunchKernelGGL((adamw_q8_multi_kernel<SDNQ_BF16>), grid, dim3(AW_BLOCK), 0, s, tab); break;
                default: hipLaunchKernelGGL((adamw_q8_multi_kernel<SDNQ_F16>), grid, dim3(AW_BLOCK), 0, s, tab); break;
            }
        });
}
