// What the units that read an SdnqWeight share -- dequant.hip and skinny.hip: the kernel view of an SdnqWeight (DeqParams, filled
// and checked by fill_params), the 16-element dequantizer every kernel on stored codes is built on, the 16-value row load and the
// host helpers of the launchers.  One definition each.  Folding a site into a helper must leave the kernel's instructions as they were
// (tools/compare_kernels.py, profiles/weight_dev_kernel_compare.txt).  Where it did not, the site keeps its own spelling: the wave-sum
// epilogue of the three linear_skinny* kernels and the `red` reduction of the two skinny_svd* kernels (skinny.hip) -- through a shared
// force-inlined helper every one of those 60 kernels came out with different instructions or registers.
#pragma once
#include <type_traits>

#include "sdnq_dev.h"
#include "unpack_dev.h"

namespace {

struct DeqParams {
    const void* w;
    const float* scale;
    const float* zp;
    const void* svd_up;    // [N][R]
    const void* svd_down;  // [R][K]
    int64_t N, K;
    int group_size, G, rank;
    int P, SG;  // conv weights: kernel positions per channel (1 for Linear) and scales per output row (G * P; codebooks: G * L * P)
    int sdt;    // SdnqWeight.scale_dtype: 16-bit -> the product below is rounded to it (dequantize_fp32=False)
    int L;      // SDNQ_KIND_CODEBOOK: levels per (row, group) = 2^bits, `scale` is the level table; 0 otherwise
    WeightFmt fmt;
};

// the scalar fields of a by-value DeqParams in one batch of kernarg loads (SDNQ_KERNARGS_NOW, sdnq_dev.h)
#define SDNQ_DEQ_ARGS_NOW(p)                                                                                                              \
    SDNQ_KERNARGS_NOW("s"((p).w), "s"((p).scale), "s"((p).zp), "s"((p).svd_up), "s"((p).svd_down), "s"((p).N), "s"((p).K), "s"((p).group_size), \
                      "s"((p).G), "s"((p).rank), "s"((p).P), "s"((p).SG), "s"((p).sdt))

// dequantize 16 elements (row n, columns k0..k0+15) to fp32: f32(w)*s or fma(f32(w), s, zp); codebooks: levels[n][g][code]
__device__ __forceinline__ void dequant16(const DeqParams& p, int64_t n, int64_t k0, float (&v)[16]) {
    load16_values(p.w, n * p.K + k0, p.fmt, v);
    const float* srow = p.scale + n * p.SG;
    const float* zrow = p.zp ? p.zp + n * p.SG : nullptr;
    if (p.L) {
        // codebook (dequantize_codebook, dequantizer.py:88-131): scale.gather along the reduction axis.  The code (< L, exact in
        // v[j]) indexes the level row of its group: [G][L] per output row, [G][L][P] for conv weights.  The levels are values of
        // the scale dtype already, so the rounding below is the identity on them.
        if (p.P > 1) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = (int)(k0 + j), c = k / p.P;
                v[j] = srow[((c / p.group_size) * p.L + (int)v[j]) * p.P + (k - c * p.P)];
            }
        } else if ((p.group_size & 15) == 0) {  // one group covers the whole 16-run (wave-uniform branch)
            const float* lrow = srow + (int)(k0 / p.group_size) * p.L;
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = lrow[(int)v[j]];
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = srow[(int)((k0 + j) / p.group_size) * p.L + (int)v[j]];
        }
    } else if (p.P > 1) {
        // conv weight [C_out][C_in][positions] quantized along C_in (quantizer.py:120-123, 205-209): one scale per
        // (output channel, channel group, kernel position); flattened k = c * P + pos
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = (int)(k0 + j), c = k / p.P;
            const int g = (c / p.group_size) * p.P + (k - c * p.P);
            v[j] = zrow ? fmaf(v[j], srow[g], zrow[g]) : v[j] * srow[g];
        }
    } else if ((p.group_size & 15) == 0) {  // one group covers the whole 16-run (wave-uniform branch)
        int64_t g64, grem;
        divmod(k0, p.group_size, g64, grem);
        const int g = (int)g64;
        const float s = srow[g];
        if (zrow) {
            const float z = zrow[g];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = fmaf(v[j], s, z);  // torch.addcmul == single-rounding fma
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = v[j] * s;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int g = (int)((k0 + j) / p.group_size);
            v[j] = zrow ? fmaf(v[j], srow[g], zrow[g]) : v[j] * srow[g];
        }
    }
    if (p.sdt != SDNQ_F32) {
        // scale / zero_point stored in the model dtype: weight.to(scale.dtype).mul_(scale) / addcmul on 16-bit tensors compute in
        // fp32 and round ONCE to that dtype (dequantizer.py:27, 63); w * s is exact in fp32, so this is that one rounding
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = round_rt(v[j], p.sdt);
    }
}

// 16 consecutive values of a float row -- base[i .. i + 15] -- as fp32: two 16-byte loads (four for float32), i % 8 == 0
template <int T_ID>
__device__ __forceinline__ void load_row16(const void* base, int64_t i, float (&v)[16]) {
    if constexpr (T_ID == SDNQ_F32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) Vec16<SDNQ_F32>::unpack(*(const uint4*)((const float*)base + i + 4 * q), v + 4 * q);
    } else {
        Vec16<T_ID>::unpack(*(const uint4*)((const uint16_t*)base + i), v);
        Vec16<T_ID>::unpack(*(const uint4*)((const uint16_t*)base + i + 8), v + 8);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
int fill_params(const SdnqWeight* w, DeqParams& p) {
    if (!w || !w->weight || !w->scale) return SDNQ_ERR_NULL;
    const int pos = w->positions > 1 ? w->positions : 1;
    if (w->n <= 0 || w->k <= 0 || w->group_size <= 0 || (w->k % pos) != 0 || ((w->k / pos) % w->group_size) != 0) return SDNQ_ERR_SHAPE;
    if ((w->k % 16) != 0) return SDNQ_ERR_SHAPE;
    if (w->storage < 0 || w->storage > 3 || w->kind < 0 || w->kind > SDNQ_KIND_CODEBOOK) return SDNQ_ERR_DTYPE;
    if (w->kind == SDNQ_KIND_CODEBOOK) {  // 2^bits levels per group, packed 1..7-bit or raw 8-bit codes, no zero point
        if (w->bits < 1 || w->bits > 8 || w->native_float) return SDNQ_ERR_DTYPE;
        if (w->storage != (w->bits == 8 ? SDNQ_ST_RAW8 : SDNQ_ST_PACKED_U8)) return SDNQ_ERR_DTYPE;
        if (w->zero_point) return SDNQ_ERR_UNSUPPORTED;
    }
    if (w->bits < 1 || w->bits > 16) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_PACKED_U8 && w->bits > 7) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_PACKED_I16 && (w->bits < 9 || w->bits > 15)) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_RAW8 && w->bits != 8) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_RAW16 && w->bits != 16) return SDNQ_ERR_DTYPE;
    if ((w->kind == SDNQ_KIND_UINT || w->kind == SDNQ_KIND_UFLOAT) && !w->zero_point) return SDNQ_ERR_NULL;
    if ((w->kind == SDNQ_KIND_FLOAT || w->kind == SDNQ_KIND_UFLOAT) && !w->native_float) {
        const int sign = (w->kind == SDNQ_KIND_FLOAT) ? 1 : 0;
        if (w->exponent < 1 || w->exponent > 7 || w->mantissa < 0 || sign + w->exponent + w->mantissa != w->bits) return SDNQ_ERR_DTYPE;
    }
    if ((uintptr_t)w->weight % 16) return SDNQ_ERR_ALIGN;
    if ((w->svd_up == nullptr) != (w->svd_down == nullptr)) return SDNQ_ERR_NULL;
    if (w->svd_up && (w->svd_rank <= 0 || w->svd_dtype < 0 || w->svd_dtype > 2)) return SDNQ_ERR_SHAPE;
    p.w = w->weight; p.scale = w->scale; p.zp = w->zero_point; p.svd_up = w->svd_up; p.svd_down = w->svd_down;
    p.N = w->n; p.K = w->k; p.group_size = w->group_size; p.G = (w->k / pos) / w->group_size; p.rank = w->svd_rank;
    p.P = pos; p.L = w->kind == SDNQ_KIND_CODEBOOK ? 1 << w->bits : 0; p.SG = p.G * pos * (p.L ? p.L : 1);
    if (w->scale_dtype < 0 || w->scale_dtype > 2) return SDNQ_ERR_DTYPE;
    p.sdt = w->scale_dtype;
    p.fmt = WeightFmt{w->storage, w->kind, w->bits, w->exponent, w->mantissa, w->native_float};
    return SDNQ_OK;
}

// 8: raw 8-bit integer codes, 4: packed 4-bit integer codes (signed or unsigned) -- what the tuned few-row kernels read; 0: anything else
inline int int_code_bits(const DeqParams& p) {
    if (p.fmt.kind != SDNQ_KIND_INT && p.fmt.kind != SDNQ_KIND_UINT) return 0;
    if (p.fmt.storage == SDNQ_ST_RAW8) return 8;
    return p.fmt.storage == SDNQ_ST_PACKED_U8 && p.fmt.bits == 4 ? 4 : 0;
}

// Run-time value -> template argument: f(std::integral_constant<int, V>{}) for the V among Vs that equals v.  False when there is none
// or f returns false, so nested calls and `if constexpr` filters compose; f is instantiated for every V, used or not.
template <int... Vs, typename F>
inline bool dispatch_int(int v, F&& f) {
    return ((v == Vs && f(std::integral_constant<int, Vs>{})) || ...);
}
template <typename F>
inline bool dispatch_float(int dtype, F&& f) {
    return dispatch_int<SDNQ_F32, SDNQ_BF16, SDNQ_F16>(dtype, f);
}

}  // namespace
