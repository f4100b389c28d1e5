// What the fused activation kernels share (actquant.hip and its rotated form actquant_had.hip): the activations on the hardware
// exponential and reciprocal, the rounded y of 8 elements, and the entry points' argument checks -- ONE implementation, so the y of the
// two entry points cannot differ by a bit.  The forms and their error bounds: the head of actquant.hip.
#pragma once
#include "rowvec_dev.h"
#include "sdnq_dev.h"

constexpr int ACT_GELU = 0, ACT_GELU_TANH = 1, ACT_SILU = 2;
constexpr double kLog2e = 1.4426950408889634, kSqrt2OverPi = 0.7978845608028654, kRsqrt2 = 0.7071067811865476;

__device__ __forceinline__ pv2f splat(float v) { return (pv2f){v, v}; }
__device__ __forceinline__ pv2f exp2_2(pv2f t) { return (pv2f){__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])}; }
__device__ __forceinline__ pv2f rcp_2(pv2f d) { return (pv2f){__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])}; }

// act(a) of two elements in float32 (the forms and their error bounds: head comment of actquant.hip)
template <int ACT>
__device__ __forceinline__ pv2f act2(pv2f a) {
    if constexpr (ACT == ACT_SILU) {
        return a * rcp_2(exp2_2(a * splat((float)-kLog2e)) + splat(1.0f));
    } else if constexpr (ACT == ACT_GELU_TANH) {
        constexpr float c0 = (float)(2.0 * kSqrt2OverPi * kLog2e), c1 = (float)(2.0 * kSqrt2OverPi * kLog2e * 0.044715);
        const pv2f p = __builtin_elementwise_fma(a * a, splat(-c1), splat(-c0));
        return a * rcp_2(exp2_2(a * p) + splat(1.0f));
    } else {
        constexpr float pc = (float)(0.3275911 * kRsqrt2);
        constexpr float h1 = (float)(0.254829592 / 2), h2 = (float)(-0.284496736 / 2), h3 = (float)(1.421413741 / 2),
                        h4 = (float)(-1.453152027 / 2), h5 = (float)(1.061405429 / 2);
        const pv2f t = rcp_2(__builtin_elementwise_fma(__builtin_elementwise_abs(a), splat(pc), splat(1.0f)));
        pv2f q = __builtin_elementwise_fma(t, splat(h5), splat(h4));
        q = __builtin_elementwise_fma(t, q, splat(h3));
        q = __builtin_elementwise_fma(t, q, splat(h2));
        q = __builtin_elementwise_fma(t, q, splat(h1));
        const pv2f e = (t * q) * exp2_2((a * a) * splat((float)(-kLog2e / 2)));
        const pv2f phi = {a[0] < 0.0f ? e[0] : 1.0f - e[0], a[1] < 0.0f ? e[1] : 1.0f - e[1]};
        return a * phi;
    }
}

// the rounded y of the 8 elements a lane owns in one pass, packed as it is stored; lanes past the end of the row (`ok` false) get zeros
template <int T_ID, int ACT, bool GATED>
__device__ __forceinline__ uint4 act8(const uint4& ra, const uint4& rb, bool ok) {
    float a[8], b[8], z[8];
    unpack8<T_ID>(ra, ra, ok, a);
    if constexpr (GATED) unpack8<T_ID>(rb, rb, ok, b);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        pv2f g = act2<ACT>((pv2f){a[2 * h], a[2 * h + 1]});
        if constexpr (GATED) g = g * (pv2f){b[2 * h], b[2 * h + 1]};
        z[2 * h] = g[0];
        z[2 * h + 1] = g[1];
    }
    return Vec16<T_ID>::pack(z);
}

// the lane vector at element `idx` of a row; UNCONDITIONAL, as load8_raw (rowvec_dev.h): a lane past the end re-reads the row's start
__device__ __forceinline__ uint4 load_raw(const void* row, int64_t idx, bool ok) { return *(const uint4*)((const uint16_t*)row + (ok ? idx : 0)); }

// host: the argument checks of sdnq_hip_act_rowquant and sdnq_hip_act_rowquant_had, in the order the statuses are documented
static inline int act_rowquant_check(const void* a, const void* b, int x_dtype, int64_t m, int64_t n, int64_t lda, int64_t ldb, int act,
                                     int mm_dtype, const void* y, const void* xq, const float* xs) {
    if (!a || (!xq != !xs) || (!xq && !y)) return SDNQ_ERR_NULL;
    if (act != ACT_GELU && act != ACT_GELU_TANH && act != ACT_SILU) return SDNQ_ERR_UNSUPPORTED;
    if (x_dtype != SDNQ_BF16 && x_dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;  // float32 rows: not built
    if (mm_dtype != SDNQ_MM_I8 && mm_dtype != SDNQ_MM_FP8) return SDNQ_ERR_DTYPE;
    if (m <= 0 || n <= 0 || (n % 8) != 0 || lda < n || (b && ldb < n) || n >= ((int64_t)1 << 24) || m >= ((int64_t)1 << 30)) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)a % 16) || ((lda * 2) % 16) || ((uintptr_t)b % 16) || (b && ((ldb * 2) % 16)) || ((uintptr_t)xq % 16) ||
        ((uintptr_t)xs % 4) || ((uintptr_t)y % 16))
        return SDNQ_ERR_ALIGN;
    return SDNQ_OK;
}
