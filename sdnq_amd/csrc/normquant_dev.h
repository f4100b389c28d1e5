// What the fused normalisation kernels share (normquant.hip and its rotated form normquant_had.hip): the fixed-order float32 sums, the
// per-row vectors, y of 8 elements once a row's statistics are known, and the entry points' argument checks -- ONE implementation, so
// the y of the two entry points cannot differ by a bit.  The formula and its layout: the head of normquant.hip.
#pragma once
#include "rowvec_dev.h"
#include "sdnq_dev.h"

__device__ __forceinline__ float wave_sum_f32(float v) {
    return __int_as_float(wave_allreduce_i32(__float_as_int(v), [](int a, int b) { return __float_as_int(__int_as_float(a) + __int_as_float(b)); }));
}
__device__ __forceinline__ float tree8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

// 8 consecutive elements of a per-row vector (weight, bias: float32 or the row dtype; scale, shift: the row dtype) as floats
template <int T_ID>
__device__ __forceinline__ void load_vec8(const void* p, int64_t i, bool f32, float (&o)[8]) {
    if (f32) {  // wave-uniform
        Vec16<SDNQ_F32>::unpack(*(const uint4*)((const float*)p + i), o);
        Vec16<SDNQ_F32>::unpack(*(const uint4*)((const float*)p + i + 4), o + 4);
    } else {
        Vec16<T_ID>::unpack(*(const uint4*)((const uint16_t*)p + i), o);
    }
}

// what a row's elements need once its statistics are known (every branch below is wave-uniform)
struct RowNorm {
    float mean, r;
    const void *weight, *bias, *scale, *shift;  // the modulation rows of this row's batch
    bool aff_f32;
};

// y = round_T(modulate(affine((x - mean) * r))) for the 8 elements at `idx`; lanes past the end of the row get zeros
template <int T_ID>
__device__ __forceinline__ void norm8(const float (&x)[8], int64_t idx, bool ok, const RowNorm& c, float (&y)[8]) {
    const int64_t i = ok ? idx : 0;
    float w[8], b[8], sc[8], sh[8];
    if (c.weight) load_vec8<T_ID>(c.weight, i, c.aff_f32, w);
    if (c.bias) load_vec8<T_ID>(c.bias, i, c.aff_f32, b);
    if (c.scale) {
        load_vec8<T_ID>(c.scale, i, false, sc);
        load_vec8<T_ID>(c.shift, i, false, sh);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float a = (x[e] - c.mean) * c.r;
        if (c.bias) a = fmaf(a, w[e], b[e]);
        else if (c.weight) a = a * w[e];
        if (c.scale) a = fmaf(a, 1.0f + sc[e], sh[e]);
        y[e] = ok ? FT<T_ID>::round(a) : 0.0f;
    }
}

// host: the argument checks of sdnq_hip_norm_rowquant and sdnq_hip_norm_rowquant_had, in the order the statuses are documented
static inline int norm_rowquant_check(const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, int norm, float eps, const void* weight,
                                      const void* bias, int affine_dtype, const void* scale, const void* shift, int64_t rows_per_batch,
                                      int64_t ld_mod, int mm_dtype, const void* y, const void* xq, const float* xs) {
    if (!x || (!xq != !xs) || (!xq && !y)) return SDNQ_ERR_NULL;
    if ((bias && !weight) || (!scale != !shift)) return SDNQ_ERR_NULL;
    if (norm != 0 && norm != 1) return SDNQ_ERR_UNSUPPORTED;
    if (norm == 1 && bias) return SDNQ_ERR_UNSUPPORTED;  // RMSNorm has no bias
    if (x_dtype != SDNQ_BF16 && x_dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;  // float32 rows: not built
    if (mm_dtype != SDNQ_MM_I8 && mm_dtype != SDNQ_MM_FP8) return SDNQ_ERR_DTYPE;
    if (weight && affine_dtype != SDNQ_F32 && affine_dtype != x_dtype) return SDNQ_ERR_DTYPE;
    if (m <= 0 || k <= 0 || (k % 8) != 0 || ldx < k || k >= ((int64_t)1 << 24)) return SDNQ_ERR_SHAPE;
    if (!(eps >= 0.0f)) return SDNQ_ERR_SHAPE;
    if (scale && (rows_per_batch <= 0 || (m % rows_per_batch) != 0 || ld_mod < k)) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((ldx * 2) % 16) || ((uintptr_t)xq % 16) || ((uintptr_t)xs % 4) || ((uintptr_t)y % 16) ||
        ((uintptr_t)weight % 16) || ((uintptr_t)bias % 16) || ((uintptr_t)scale % 16) || ((uintptr_t)shift % 16) ||
        (scale && ((ld_mod * 2) % 16)))
        return SDNQ_ERR_ALIGN;
    return SDNQ_OK;
}
