// Fused activation (+ gate product) + ROTATED row quantization for gfx950: the y of actquant.hip, bit for bit (act8: the same float32
// operations, ONE rounding), and in the same launch the int8 / fp8 codes and row scale of rotate_hadamard(y) -- what
// sdnq_hip_rowquant(y, mm, hadamard_group) writes for that y.  The consumers are the w8a8 layers quantized with use_hadamard = True
// (FLUX int4 + Hadamard: ff.net.2 behind GELU(tanh), N = 12288).  The kernels and the choice of the re-layout between the producer's
// and the matrix cores' row layout: producer_had_dev.h.  Here: what an activated row is (ActRow), the entry point and its dispatch.
//   group 256, N <= 16384 (the row quantizer's matrix-core form): producer_had256_kernel.  N <= 4096: a row per wave, 2, 4, 6 or 8 passes
//       of both operands in flight and then in registers.  Longer rows: y needs no statistic of its row, so the row is cut over the
//       four waves of a workgroup (6 passes each up to 12288, 8 up to 16384) and only the amax meets in LDS -- every load of the row in
//       flight at once, the rotated row packed in 24 / 32 registers per lane, no LDS image of the row.
//   every other group: producer_fwht_kernel (2 or 8 passes in registers, else y and the rotation computed twice); the activation is
//       chosen at run time there (wave-uniform), to keep the number of kernels down.
#include "actquant_dev.h"
#include "producer_had_dev.h"

namespace {

struct ActHadArgs {
    const void* a;           // [M][N] of the row dtype, row stride lda elements: the operand of the activation
    const void* b;           // the multiplier, row stride ldb (GATED kernels only)
    int64_t M, N, lda, ldb;
    int act;                 // read by the kernels built with ACT == ACT_ANY
    int log2g;               // log2 of the Hadamard group
    void* y;                 // [M][N] of the row dtype or NULL
    uint8_t* xq;             // codes and row scales of the rotated row
    float* xs;
};

constexpr int ACT_ANY = -1;

// A row of the actquant kernels: NP passes of both operands from element k0 on in registers, or, NP == 0, every pass loaded where it
// is used.  y8() is act8.
template <int T_ID, int ACT, bool GATED, int NP>
struct ActRow {
    using Args = ActHadArgs;
    static constexpr int T = T_ID;
    static __device__ __forceinline__ int64_t len(const Args& A) { return A.N; }
    uint4 ra[NP > 0 ? NP : 1], rb[GATED && NP > 0 ? NP : 1];
    const void *arow, *brow;
    int act;

    __device__ __forceinline__ void begin(const Args& A, int64_t m, int64_t k0, int lane) {
        arow = (const char*)A.a + m * A.lda * 2;
        brow = GATED ? (const char*)A.b + m * A.ldb * 2 : arow;
        act = A.act;
        if constexpr (NP > 0) {  // every pass of both operands in flight before the first use
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int64_t idx = k0 + (int64_t)p * 512 + lane * 8;
                ra[p] = load_raw(arow, idx, idx < A.N);
                if constexpr (GATED) rb[p] = load_raw(brow, idx, idx < A.N);
            }
        }
    }
    __device__ __forceinline__ uint4 y8(int64_t p, int64_t idx, bool ok) const {
        uint4 va, vb;
        if constexpr (NP > 0) {
            va = ra[p];
            vb = rb[GATED ? p : 0];
        } else {
            va = load_raw(arow, idx, ok);
            vb = GATED ? load_raw(brow, idx, ok) : va;
        }
        if constexpr (ACT == ACT_ANY) {
            if (act == ACT_GELU) return act8<T_ID, ACT_GELU, GATED>(va, vb, ok);  // wave-uniform
            if (act == ACT_GELU_TANH) return act8<T_ID, ACT_GELU_TANH, GATED>(va, vb, ok);
            return act8<T_ID, ACT_SILU, GATED>(va, vb, ok);
        } else {
            return act8<T_ID, ACT, GATED>(va, vb, ok);
        }
    }
};

}  // namespace

extern "C" int sdnq_hip_act_rowquant_had(const void* a, const void* b, int x_dtype, int64_t m, int64_t n, int64_t lda, int64_t ldb, int act,
                                         int mm_dtype, int hadamard_group, void* y, void* xq, float* xs, sdnq_stream_t stream) {
    const int st = act_rowquant_check(a, b, x_dtype, m, n, lda, ldb, act, mm_dtype, y, xq, xs);
    if (st != SDNQ_OK) return st;
    const int log2g = hadamard_log2(hadamard_group, n);
    if (log2g < 0) return SDNQ_ERR_SHAPE;
    if (log2g == 0 || !xq)  // no rotation, or no codes to rotate: the plain kernels
        return sdnq_hip_act_rowquant(a, b, x_dtype, m, n, lda, ldb, act, mm_dtype, y, xq, xs, stream);
    ActHadArgs A;
    A.a = a; A.b = b; A.M = m; A.N = n; A.lda = lda; A.ldb = ldb;
    A.act = act; A.log2g = log2g;
    A.y = y; A.xq = (uint8_t*)xq; A.xs = xs;
    hipStream_t s = (hipStream_t)stream;
    const int np = (int)((n + 511) / 512);
    const bool mfma = hadamard_group == 256 && n <= 16384;  // where sdnq_hip_rowquant rotates on the matrix cores
    const bool wide = mfma && np > 8;                       // the row over the four waves of a workgroup
    dim3 grid((unsigned)(wide ? m : (m + 3) / 4)), block(256);
#define AH_256(T, MMV, ACTV, G, NPV, W) hipLaunchKernelGGL((producer_had256_kernel<ActRow<T, ACTV, G, NPV>, MMV, NPV, W>), grid, block, 0, s, A)
#define AH_NP(T, MMV, ACTV, G)                          \
    do {                                                \
        if (np <= 2) AH_256(T, MMV, ACTV, G, 2, 1);      \
        else if (np <= 4) AH_256(T, MMV, ACTV, G, 4, 1); \
        else if (np <= 6) AH_256(T, MMV, ACTV, G, 6, 1); \
        else if (np <= 8) AH_256(T, MMV, ACTV, G, 8, 1); \
        else if (np <= 24) AH_256(T, MMV, ACTV, G, 6, 4); \
        else AH_256(T, MMV, ACTV, G, 8, 4);              \
    } while (0)
#define AH_ACT(T, MMV, G)                                           \
    do {                                                            \
        if (act == ACT_GELU) AH_NP(T, MMV, ACT_GELU, G);            \
        else if (act == ACT_GELU_TANH) AH_NP(T, MMV, ACT_GELU_TANH, G); \
        else AH_NP(T, MMV, ACT_SILU, G);                            \
    } while (0)
#define AH_FWHT(T, MMV, G, NPV) hipLaunchKernelGGL((producer_fwht_kernel<ActRow<T, ACT_ANY, G, NPV>, MMV, NPV>), grid, block, 0, s, A)
#define AH_FORM(T, MMV, G)                         \
    do {                                           \
        if (mfma) AH_ACT(T, MMV, G);               \
        else if (np <= 2) AH_FWHT(T, MMV, G, 2);   \
        else if (np <= 8) AH_FWHT(T, MMV, G, 8);   \
        else AH_FWHT(T, MMV, G, 0);                \
    } while (0)
#define AH_G(T, MMV) do { if (b) AH_FORM(T, MMV, true); else AH_FORM(T, MMV, false); } while (0)
#define AH_MM(T) do { if (mm_dtype == SDNQ_MM_I8) AH_G(T, SDNQ_MM_I8); else AH_G(T, SDNQ_MM_FP8); } while (0)
    if (x_dtype == SDNQ_BF16) AH_MM(SDNQ_BF16);
    else AH_MM(SDNQ_F16);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
