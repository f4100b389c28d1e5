// Fused normalisation + ROTATED row quantization for gfx950: the y of normquant.hip, bit for bit (the same statistics in the same
// order, norm8, ONE rounding), and in the same launch the int8 / fp8 codes and row scale of rotate_hadamard(y) -- what
// sdnq_hip_rowquant(y, mm, hadamard_group) writes for that y.  The consumers are the w8a8 layers quantized with use_hadamard = True
// (FLUX int4 + Hadamard: every Linear behind an adaLN LayerNorm); today they read y back and run the rotated row quantizer themselves.
// The kernels and the choice of the re-layout between the producer's and the matrix cores' row layout: producer_had_dev.h.  Here: what
// a normalised row is (NormRow), the entry point and its dispatch.
//   group 256, K <= 16384 (the row quantizer's matrix-core form): producer_had256_kernel, rows up to 4096 in registers (2, 4, 6, 8
//       passes), longer ones as the sweep form (every pass re-read from L2, y and the rotation computed twice).  A row's sums run
//       over all its passes per lane, in order: a row cannot be split over waves without changing the bits of y.
//   every other group: producer_fwht_kernel (2, 4, 8 passes in registers, else the sweep form).
#include "normquant_dev.h"
#include "producer_had_dev.h"

namespace {

struct NormHadArgs {
    const void* x;
    int64_t M, K, ldx;
    int rms;                 // 0 LayerNorm, 1 RMSNorm
    float eps;
    int aff_f32;             // weight / bias are float32 (else the row dtype)
    int log2g;               // log2 of the Hadamard group
    const void* weight;      // [K] or NULL
    const void* bias;        // [K] or NULL
    const void* scale;       // [B][ld_mod] of the row dtype or NULL
    const void* shift;
    int64_t rows_per_batch, ld_mod;
    void* y;                 // [M][K] of the row dtype or NULL
    uint8_t* xq;             // codes and row scales of the rotated row
    float* xs;
};

// A row of normquant_kernel: NP passes in registers (K <= NP * 512) or, NP == 0, every pass re-read.  begin() is that kernel's
// statistics, statement for statement; y8() its norm8.
template <int T_ID, int NP>
struct NormRow {
    using Args = NormHadArgs;
    static constexpr int T = T_ID;
    static __device__ __forceinline__ int64_t len(const Args& A) { return A.K; }
    float v[NP > 0 ? NP : 1][8];
    const void* row;
    int64_t K;
    int lane;
    RowNorm c;

    __device__ __forceinline__ void x8(int64_t p, float (&t)[8]) const {  // pass p of the input row
        if constexpr (NP > 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] = v[p][e];
        } else {
            const int64_t idx = p * 512 + lane * 8;
            load8<T_ID>(row, idx, idx < K, t);
        }
    }
    __device__ __forceinline__ void begin(const Args& A, int64_t m, int64_t, int lane_) {
        lane = lane_;
        K = A.K;
        row = (const char*)A.x + m * A.ldx * 2;
        const int64_t npass = NP > 0 ? NP : (K + 511) / 512;
        constexpr int UNR = NP > 0 ? NP : 1;
        if constexpr (NP > 0) {
            uint4 ra[NP], rb[NP];  // every pass of the row in flight before the first use
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int64_t idx = (int64_t)p * 512 + lane * 8;
                load8_raw<T_ID>(row, idx, idx < K, ra[p], rb[p]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) unpack8<T_ID>(ra[p], rb[p], (int64_t)p * 512 + lane * 8 < K, v[p]);
        }
        const float fk = (float)K;
        c.mean = 0.0f;
        if (!A.rms) {
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll UNR
            for (int64_t p = 0; p < npass; ++p) {
                float t[8];
                x8(p, t);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += t[e];  // (lanes past the end hold zeros)
            }
            c.mean = wave_sum_f32(tree8(acc)) / fk;
        }
        {
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll UNR
            for (int64_t p = 0; p < npass; ++p) {
                float t[8];
                x8(p, t);
                const bool ok = p * 512 + lane * 8 < K;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = t[e] - c.mean;
                    acc[e] += ok ? d * d : 0.0f;
                }
            }
            const float var = wave_sum_f32(tree8(acc)) / fk;
            c.r = 1.0f / sqrtf(var + A.eps);
        }
        c.weight = A.weight;
        c.bias = A.bias;
        c.aff_f32 = A.aff_f32 != 0;
        c.scale = c.shift = nullptr;
        if (A.scale) {
            int64_t b, rem;
            divmod(m, A.rows_per_batch, b, rem);
            c.scale = (const char*)A.scale + b * A.ld_mod * 2;
            c.shift = (const char*)A.shift + b * A.ld_mod * 2;
        }
    }
    __device__ __forceinline__ uint4 y8(int64_t p, int64_t idx, bool ok) const {
        float t[8], yv[8];
        x8(p, t);
        norm8<T_ID>(t, idx, ok, c, yv);
        return Vec16<T_ID>::pack(yv);  // (rounded already: the bits store8 writes)
    }
};

}  // namespace

extern "C" int sdnq_hip_norm_rowquant_had(const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, int norm, float eps,
                                          const void* weight, const void* bias, int affine_dtype,
                                          const void* scale, const void* shift, int64_t rows_per_batch, int64_t ld_mod,
                                          int mm_dtype, int hadamard_group, void* y, void* xq, float* xs, sdnq_stream_t stream) {
    const int st = norm_rowquant_check(x, x_dtype, m, k, ldx, norm, eps, weight, bias, affine_dtype, scale, shift, rows_per_batch, ld_mod, mm_dtype,
                                       y, xq, xs);
    if (st != SDNQ_OK) return st;
    const int log2g = hadamard_log2(hadamard_group, k);
    if (log2g < 0) return SDNQ_ERR_SHAPE;
    if (log2g == 0 || !xq)  // no rotation, or no codes to rotate: the plain kernels
        return sdnq_hip_norm_rowquant(x, x_dtype, m, k, ldx, norm, eps, weight, bias, affine_dtype, scale, shift, rows_per_batch, ld_mod, mm_dtype,
                                      y, xq, xs, stream);
    NormHadArgs a;
    a.x = x; a.M = m; a.K = k; a.ldx = ldx;
    a.rms = norm; a.eps = eps;
    a.aff_f32 = affine_dtype == SDNQ_F32;
    a.log2g = log2g;
    a.weight = weight; a.bias = bias; a.scale = scale; a.shift = shift;
    a.rows_per_batch = rows_per_batch; a.ld_mod = ld_mod;
    a.y = y; a.xq = (uint8_t*)xq; a.xs = xs;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((m + 3) / 4)), block(256);
    const int np = (int)((k + 511) / 512);
    const bool mfma = hadamard_group == 256 && k <= 16384;  // where sdnq_hip_rowquant rotates on the matrix cores
#define NH_256(T, MMV, NPV) hipLaunchKernelGGL((producer_had256_kernel<NormRow<T, NPV>, MMV, NPV, 1>), grid, block, 0, s, a)
#define NH_FWHT(T, MMV, NPV) hipLaunchKernelGGL((producer_fwht_kernel<NormRow<T, NPV>, MMV, NPV>), grid, block, 0, s, a)
#define NH_NP(T, MMV)                             \
    do {                                          \
        if (mfma) {                               \
            if (np <= 2) NH_256(T, MMV, 2);       \
            else if (np <= 4) NH_256(T, MMV, 4);  \
            else if (np <= 6) NH_256(T, MMV, 6);  \
            else if (np <= 8) NH_256(T, MMV, 8);  \
            else NH_256(T, MMV, 0);               \
        } else {                                  \
            if (np <= 2) NH_FWHT(T, MMV, 2);      \
            else if (np <= 4) NH_FWHT(T, MMV, 4); \
            else if (np <= 8) NH_FWHT(T, MMV, 8); \
            else NH_FWHT(T, MMV, 0);              \
        }                                         \
    } while (0)
#define NH_MM(T) do { if (mm_dtype == SDNQ_MM_I8) NH_NP(T, SDNQ_MM_I8); else NH_NP(T, SDNQ_MM_FP8); } while (0)
    if (x_dtype == SDNQ_BF16) NH_MM(SDNQ_BF16);
    else NH_MM(SDNQ_F16);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
