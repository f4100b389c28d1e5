// What the adapter units (lowrank_train.hip, conv_lowrank.hip) share: the 16x16x32 MFMA of both 16-bit formats, the swizzled LDS images
// that ds_read_b64_tr_b16 reads transposed, and the second launch of the deterministic factor gradients.
#pragma once
#include "sdnq_dev.h"

namespace {

typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s* lds_v4s_ptr;

template <bool IS_BF16>
__device__ __forceinline__ v4f mfma16(v4i a, v4i b, v4f c) {
    if constexpr (IS_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

// LDS images of rows of 32 NP bytes; the 32-byte column pair cp of row i lies at pair cp ^ lrg_swz<NP>(i) (the bank arithmetic is in
// lowrank_train.hip's header comment)
template <int NRT> __device__ __forceinline__ int lrg_swz(int i) {
    if constexpr (NRT == 1) return 0;
    else if constexpr (NRT == 2) return (i >> 3) & 1;
    else if constexpr (NRT == 4) return ((i >> 1) & 1) | (((i >> 3) & 1) << 1);
    else return (i & 3) | (((i >> 3) & 1) << 2);
}

// the fragment of v_mfma_f32_16x16x32 (A or B alike) for 32 rows i0 .. i0 + 31 and 16 columns of a [rows][16 NP columns] LDS image:
// lane l gets rows i0 + 8 (l / 16) + 0..7 of column l % 16.  Two transposed reads of 4 rows each; lane 4 q + p of a 16-lane group supplies
// the address of row q, columns 4 p .. 4 p + 3 of the block.
template <int NP>
__device__ __forceinline__ v4i lrg_frag(const uint8_t* img, int i0, int cp, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int r0 = i0 + 8 * g + q, r1 = r0 + 4;
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_ptr)(img + r0 * (NP * 32) + ((cp ^ lrg_swz<NP>(r0)) << 5) + 8 * p));
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_ptr)(img + r1 * (NP * 32) + ((cp ^ lrg_swz<NP>(r1)) << 5) + 8 * p));
    const v2i l2 = __builtin_bit_cast(v2i, lo), h2 = __builtin_bit_cast(v2i, hi);
    return (v4i){l2[0], l2[1], h2[0], h2[1]};
}

// out[j][r] (or [r][j]) = round( scale * (((part[0] + part[1]) + part[2]) + ...) ) of part [slab][P][R]: one thread per element, slabs in
// ascending order
__global__ __launch_bounds__(256) void lowrank_grad_sum_kernel(const float* __restrict__ part, int64_t slabs, int64_t P, int R, float scale,
                                                               int out_t, void* __restrict__ out, int out_dtype) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x, total = P * R;
    if (o >= total) return;
    float s = part[o];
    for (int64_t k = 1; k < slabs; ++k) s += part[k * total + o];
    const int64_t j = o / R, r = o % R;
    st_rt(out, out_t ? r * P + j : o, scale * s, out_dtype);
}

}  // namespace
