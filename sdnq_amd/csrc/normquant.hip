// Fused normalisation + row quantization for gfx950: LayerNorm / RMSNorm (+ affine, + adaLN modulation) of an activation row, the ONE
// rounding to the row dtype, and the int8 / fp8 codes and row scale the row quantizer (rowquant.hip) would write for that rounded row
// -- one launch where the norm is a float kernel that writes y and the quantizer a second launch that reads y back.
//
//   stats (float32): LayerNorm: mean = sum(x) / K, var = sum((x - mean)^2) / K (two-pass, from the registers);  RMSNorm: ms = sum(x^2) / K
//   r = 1 / sqrt(var + eps)                                   IEEE sqrt and division
//   n = (x - mean) * r                                        (RMSNorm: mean = 0, x - 0 is x)
//   a = fmaf(n, weight, bias) | n * weight | n
//   z = fmaf(a, 1 + scale[b], shift[b]) | a                   b = row / rows_per_batch
//   y = round_T(z);   xs = amax|y| / qmax;   xq = quant8(y / xs)     the quantizer's own arithmetic (quant8_dev.h)
//
// HBM-bound: reads 2 B and writes 1 B (+ 2 B with the y store) per element, + 4 B per row; the per-row vectors stay in L2.
// Layout: the row quantizer's -- one wave (64 lanes) per row, 8 consecutive elements per lane per 512-element pass, every global
// access a 16-byte lane vector (rowvec_dev.h).  Rows up to NP * 512 <= 4096 elements live in registers across the three reductions
// (sum, sum of squared deviations, amax|y|); the normalised row replaces the input row in the same registers, so the row is read
// from HBM once.  Longer rows (NP == 0) take the sweep form: the same code with every pass re-read from L2 and y recomputed for the
// codes (same inputs, same operations: the same bits).  No LDS.
// Every sum runs in a fixed order -- 8 per-lane accumulators over the passes, a tree over the 8, the xor butterfly over the lanes -- and
// a row never leaves its wave, so a row's bits do not depend on M or the grid.
#include "normquant_dev.h"
#include "quant8_dev.h"
#include "rowvec_dev.h"
#include "sdnq_dev.h"

namespace {

struct NormQuantArgs {
    const void* x;
    int64_t M, K, ldx;
    int row_blocks;
    int rms;                 // 0 LayerNorm, 1 RMSNorm
    float eps;
    int aff_f32;             // weight / bias are float32 (else the row dtype)
    const void* weight;      // [K] or NULL
    const void* bias;        // [K] or NULL
    const void* scale;       // [B][ld_mod] of the row dtype or NULL
    const void* shift;
    int64_t rows_per_batch, ld_mod;
    void* y;                 // [M][K] of the row dtype or NULL
    uint8_t* xq;             // codes and row scales: both, or both NULL (then only y is written)
    float* xs;
    const uint4* pf;         // NULL / 0: no entry point takes a prefetch operand (rowvec_dev.h: prefetch_block)
    int64_t pf_vecs;
};

// T_ID: row dtype (bf16 / f16); MM: SdnqMM; NP: 512-element passes of the row held in registers (K <= NP * 512), 0: the sweep form
template <int T_ID, int MM, int NP>
__global__ __launch_bounds__(256) void normquant_kernel(const NormQuantArgs A) {
    if ((int)blockIdx.x >= A.row_blocks) {
        prefetch_block(A.pf, A.pf_vecs, (int64_t)blockIdx.x - A.row_blocks, A.xs);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= A.M) return;  // whole wave exits together
    const int64_t K = A.K;
    const void* row = (const char*)A.x + m * A.ldx * 2;
    const int64_t npass = NP > 0 ? NP : (K + 511) / 512;
    constexpr int UNR = NP > 0 ? NP : 1;  // the pass loops: unrolled over the registers, a plain loop in the sweep form
    float v[NP > 0 ? NP : 1][8];
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
    // pass p of the row: from the registers, or read again (L2)
    auto pass = [&](int64_t p, float (&t)[8]) {
        if constexpr (NP > 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] = v[p][e];
        } else {
            const int64_t idx = p * 512 + lane * 8;
            load8<T_ID>(row, idx, idx < K, t);
        }
    };
    const float fk = (float)K;
    RowNorm c;
    c.mean = 0.0f;
    if (!A.rms) {
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll UNR
        for (int64_t p = 0; p < npass; ++p) {
            float t[8];
            pass(p, t);
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
            pass(p, t);
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
    void* yrow = A.y ? (char*)A.y + m * K * 2 : nullptr;
    float amax = 0.0f;
#pragma unroll UNR
    for (int64_t p = 0; p < npass; ++p) {
        const int64_t idx = p * 512 + lane * 8;
        const bool ok = idx < K;
        float t[8], yv[8];
        pass(p, t);
        norm8<T_ID>(t, idx, ok, c, yv);
        if (yrow && ok) store8<T_ID>(yrow, idx, yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            amax = fmaxf(amax, fabsf(yv[e]));
            if constexpr (NP > 0) v[p][e] = yv[e];  // the normalised row takes the input row's registers
        }
    }
    if (A.xq == nullptr) return;  // only y was asked for
    RowDiv rd;
    rd.set(row_scale<MM>(amax, lane, A.xs + m));
    uint8_t* qrow = A.xq + m * K;
    int isum = 0;  // (quant8's row sum: unused here)
#pragma unroll UNR
    for (int64_t p = 0; p < npass; ++p) {
        const int64_t idx = p * 512 + lane * 8;
        const bool ok = idx < K;
        float yv[8];
        if constexpr (NP > 0) {
            pass(p, yv);
        } else {
            float t[8];
            pass(p, t);
            norm8<T_ID>(t, idx, ok, c, yv);
        }
        if (ok) store_codes8(qrow + idx, quant8<MM>(yv, rd, isum));
    }
}

}  // namespace

extern "C" int sdnq_hip_norm_rowquant(const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, int norm, float eps,
                                      const void* weight, const void* bias, int affine_dtype,
                                      const void* scale, const void* shift, int64_t rows_per_batch, int64_t ld_mod,
                                      int mm_dtype, void* y, void* xq, float* xs, sdnq_stream_t stream) {
    const int st = norm_rowquant_check(x, x_dtype, m, k, ldx, norm, eps, weight, bias, affine_dtype, scale, shift, rows_per_batch, ld_mod, mm_dtype,
                                       y, xq, xs);
    if (st != SDNQ_OK) return st;
    NormQuantArgs a;
    a.x = x; a.M = m; a.K = k; a.ldx = ldx;
    a.row_blocks = (int)((m + 3) / 4);
    a.rms = norm; a.eps = eps;
    a.aff_f32 = affine_dtype == SDNQ_F32;
    a.weight = weight; a.bias = bias; a.scale = scale; a.shift = shift;
    a.rows_per_batch = rows_per_batch; a.ld_mod = ld_mod;
    a.y = y; a.xq = (uint8_t*)xq; a.xs = xs;
    a.pf = nullptr; a.pf_vecs = 0;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)a.row_blocks), block(256);
    const int np = (int)((k + 511) / 512);
#define NQ_LAUNCH(T, MMV, NPV) hipLaunchKernelGGL((normquant_kernel<T, MMV, NPV>), grid, block, 0, s, a)
#define NQ_NP(T, MMV)                           \
    do {                                        \
        if (np <= 1) NQ_LAUNCH(T, MMV, 1);      \
        else if (np <= 2) NQ_LAUNCH(T, MMV, 2); \
        else if (np <= 3) NQ_LAUNCH(T, MMV, 3); \
        else if (np <= 5) NQ_LAUNCH(T, MMV, 5); \
        else if (np <= 6) NQ_LAUNCH(T, MMV, 6); \
        else if (np <= 8) NQ_LAUNCH(T, MMV, 8); \
        else NQ_LAUNCH(T, MMV, 0);              \
    } while (0)
#define NQ_MM(T) do { if (mm_dtype == SDNQ_MM_I8) NQ_NP(T, SDNQ_MM_I8); else NQ_NP(T, SDNQ_MM_FP8); } while (0)
    if (x_dtype == SDNQ_BF16) NQ_MM(SDNQ_BF16);
    else NQ_MM(SDNQ_F16);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
