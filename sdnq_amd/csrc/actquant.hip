// Fused activation + row quantization for gfx950: GELU / GELU(tanh) / SiLU of an activation row, the optional gate product (GEGLU,
// SwiGLU), the ONE rounding to the row dtype, and the int8 / fp8 codes and row scale the row quantizer (rowquant.hip) would write for
// that rounded row -- one launch where torch runs chunk + activation + mul (two or three elementwise passes and a [M][N] temporary)
// and the quantizer a launch of its own that reads y back.
//
//   g = act(a)  (float32, forms below);   z = g * b | g;   y = round_T(z);   xs = amax|y| / qmax;   xq = quant8(y / xs)   (quant8_dev.h)
//
// Layout: the row quantizer's -- one wave (64 lanes) per row, 8 consecutive elements per lane per 512-element pass, every global
// access a 16-byte lane vector.  The only reduction is amax|y| (a per-lane fmaxf over the passes in order, then the xor butterfly),
// and a row never leaves its wave: a row's bits do not depend on M or the grid.  Three forms by row length, all the same operations:
//   N <= 4096 (actquant_reg_kernel, NP = 1, 2, 3, 5, 8 passes): every load of the row in flight at once, the rounded y PACKED (2 B per
//       element) in registers between the amax reduction and the encode step; four rows per 256-thread workgroup.
//   N <= 16384 (actquant_long_kernel, LDS): the packed y goes to a wave-private LDS image of the row, 2 B per element, and comes back
//       for the encode step; a lane reads only what it wrote itself, so there is no barrier.  ONE wave per workgroup, so the LDS a CU
//       can hold (160 KB) bounds the waves per CU directly: 2N bytes per wave leave 6 waves per CU at the FLUX row (12288), 5 at 14336
//       and 16384 (a four-wave workgroup would fit once: 4 waves).  With four passes of both operands in flight per wave (8 KB) five
//       waves per CU still keep ~10 MB in flight on 256 CUs -- what HBM needs.  Past 16384 that drops to 4 waves and less:
//   N > 16384 (the same kernel, no LDS): the second sweep re-reads a and b (L2) and recomputes y -- same inputs, same operations, the
//       same bits, at twice the ALU cost.
//
// ALU budget: the gated form moves 4 B in and 1-3 B out per element; at HBM speed that leaves ~20 lane-issue slots per element, of which
// unpack, gate, pack, amax and the encode step take ~8.  A libm erff / tanhf (30-60 instructions) does not fit, so the activations are
// written on the hardware's v_exp_f32 (2^x) and v_rcp_f32, both documented at 1 ulp, and the multiplies / fmas as packed pairs
// (v_pk_mul_f32 / v_pk_fma_f32).  With u = 2^-24 (half an ulp of float32), errors as multiples of u * |a|:
//   SiLU        g = a * rcp(1 + exp2(-log2e * a))
//               exponent: constant u + product u, an absolute 2u|a| in the exponential's argument; exp2 2u; 1 + e: u; rcp 2u; a * s: u.
//               With s = sigmoid(a):  |dg| <= |a| s ((1 - s)(2|a| + 2) + 4) u <= 4.95 u |a|   (|a| s (1 - s) <= 0.2239, s (1 - s) <= 1/4)
//   GELU(tanh)  0.5 a (1 + tanh w) = a * sigmoid(2w), w = sqrt(2/pi) (a + 0.044715 a^3):   g = a * rcp(1 + exp2(a * fma(a*a, -C1, -C0)))
//               exponent: a*a u, constants u, fma u, product u = 4u relative, an absolute 4u|2w|; the rest as SiLU:
//               |dg| <= |a| s ((1 - s)(4|2w| + 2) + 4) u <= 5.4 u |a|
//   GELU(erf)   0.5 a (1 + erf(a / sqrt 2)) = a * Phi(a), Abramowitz & Stegun 7.1.26:  t = rcp(1 + (p / sqrt 2) |a|),
//               E = t (h1 + t (h2 + t (h3 + t (h4 + t h5)))) * exp2(-log2e / 2 * a*a),  h_i = a_i / 2;   Phi = a < 0 ? E : 1 - E
//               (t lies in (0, 1] by construction: that is the clamp; E needs no cancellation on either side).
//               approximation: |erf error| <= 1.5e-7, half of it in Phi: 1.26 u;  t: constant u (1 - t), fma u, rcp 2u, through
//               t P'(t) <= 3.45 at weight 1/2: 5.2 u;  Horner, term i passing i + 1 roundings and its constant's:
//               sum (i + 1) |h_i| <= 10.4 u;  exponential (argument 3u relative, x^2 e^(-x^2) <= 1/e; exp2 2u): 1.6 u;
//               poly * exp 0.5 u;  1 - E u;  a * Phi u:   |dg| <= 21 u |a|
//   gate        z = g * b: one more u of |a b|.
//   ACT_ERR (below, and what tests/test_actquant_gpu.py asserts with |a| max(1, |b|)): the sums above plus the gate, rounded up to
//   leave room for the second-order terms -- SiLU 6, GELU(tanh) 7, GELU(erf) 24.  Half an ulp of f16 is 4096 u, of bf16 32768 u.
// Special values: act(+-0) = +-0 * 0.5; a large |a| overflows a*a or the exponential to inf / 0, never to NaN: rcp(inf) = 0 and
// exp2(-inf) = 0 give g = a for a > 0 and -0 for a < 0; a NaN reaches g through the last product.
#include "actquant_dev.h"
#include "quant8_dev.h"
#include "rowvec_dev.h"
#include "sdnq_dev.h"

namespace {

struct ActQuantArgs {
    const void* a;           // [M][N] of the row dtype, row stride lda elements: the operand of the activation
    const void* b;           // the multiplier, row stride ldb (GATED kernels only)
    int64_t M, N, lda, ldb;
    int row_blocks;
    int use_lds;             // actquant_long_kernel: the packed y row is held in LDS for the encode step (else recomputed)
    void* y;                 // [M][N] of the row dtype or NULL
    uint8_t* xq;             // codes and row scales: both, or both NULL (then only y is written)
    float* xs;
    const uint4* pf;         // NULL / 0: no entry point takes a prefetch operand (rowvec_dev.h: prefetch_block)
    int64_t pf_vecs;
};

constexpr int ACT_REG_MAX_N = 4096, ACT_LDS_MAX_N = 16384;

// Rows of N <= NP * 512 <= 4096.  T_ID: row dtype (bf16 / f16); MM: SdnqMM; ACT: the activation; GATED: z = act(a) * b
template <int T_ID, int MM, int ACT, bool GATED, int NP>
__global__ __launch_bounds__(256) void actquant_reg_kernel(const ActQuantArgs A) {
    if ((int)blockIdx.x >= A.row_blocks) {
        prefetch_block(A.pf, A.pf_vecs, (int64_t)blockIdx.x - A.row_blocks, A.xs);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= A.M) return;  // whole wave exits together
    const int64_t N = A.N;
    const void* arow = (const char*)A.a + m * A.lda * 2;
    const void* brow = GATED ? (const char*)A.b + m * A.ldb * 2 : arow;
    uint4 ra[NP], rb[GATED ? NP : 1];  // every pass of both operands in flight before the first use
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int64_t idx = (int64_t)p * 512 + lane * 8;
        ra[p] = load_raw(arow, idx, idx < N);
        if constexpr (GATED) rb[p] = load_raw(brow, idx, idx < N);
    }
    void* yrow = A.y ? (char*)A.y + m * N * 2 : nullptr;
    uint4 yp[NP];
    float amax = 0.0f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int64_t idx = (int64_t)p * 512 + lane * 8;
        const bool ok = idx < N;
        yp[p] = act8<T_ID, ACT, GATED>(ra[p], rb[GATED ? p : 0], ok);
        if (yrow && ok) *(uint4*)((uint16_t*)yrow + idx) = yp[p];
        float yv[8];
        Vec16<T_ID>::unpack(yp[p], yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(yv[e]));
    }
    if (A.xq == nullptr) return;  // only y was asked for
    RowDiv rd;
    rd.set(row_scale<MM>(amax, lane, A.xs + m));
    uint8_t* qrow = A.xq + m * N;
    int isum = 0;  // (quant8's row sum: unused here)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int64_t idx = (int64_t)p * 512 + lane * 8;
        float yv[8];
        Vec16<T_ID>::unpack(yp[p], yv);
        if (idx < N) store_codes8(qrow + idx, quant8<MM>(yv, rd, isum));
    }
}

// Rows of N > 4096: one wave per workgroup, U passes of both operands in flight; the packed y row in LDS (A.use_lds) or recomputed
template <int T_ID, int MM, int ACT, bool GATED>
__global__ __launch_bounds__(64) void actquant_long_kernel(const ActQuantArgs A) {
    extern __shared__ uint4 img[];  // [ceil(N / 512)][64] lane vectors of the rounded row; a lane reads back only its own
    if ((int)blockIdx.x >= A.row_blocks) {
        prefetch_block<64>(A.pf, A.pf_vecs, (int64_t)blockIdx.x - A.row_blocks, A.xs);
        return;
    }
    constexpr int U = 4;
    const int lane = threadIdx.x;
    const int64_t m = blockIdx.x;
    const int64_t N = A.N;
    const int64_t npass = (N + 511) / 512;
    const bool lds = A.use_lds != 0;
    const void* arow = (const char*)A.a + m * A.lda * 2;
    const void* brow = GATED ? (const char*)A.b + m * A.ldb * 2 : arow;
    // the packed y of passes p0 .. p0 + U - 1 from the operands (passes past the end of the row: zeros)
    auto compute = [&](int64_t p0, uint4 (&yp)[U]) {
        uint4 ra[U], rb[GATED ? U : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t idx = (p0 + u) * 512 + lane * 8;
            ra[u] = load_raw(arow, idx, idx < N);
            if constexpr (GATED) rb[u] = load_raw(brow, idx, idx < N);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) yp[u] = act8<T_ID, ACT, GATED>(ra[u], rb[GATED ? u : 0], (p0 + u) * 512 + lane * 8 < N);
    };
    void* yrow = A.y ? (char*)A.y + m * N * 2 : nullptr;
    float amax = 0.0f;
    for (int64_t p0 = 0; p0 < npass; p0 += U) {
        uint4 yp[U];
        compute(p0, yp);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t idx = (p0 + u) * 512 + lane * 8;
            const bool ok = idx < N;  // (false for every lane of a pass past the end: p0 + u < npass where it holds)
            if (lds && ok) img[(p0 + u) * 64 + lane] = yp[u];
            if (yrow && ok) *(uint4*)((uint16_t*)yrow + idx) = yp[u];
            float yv[8];
            Vec16<T_ID>::unpack(yp[u], yv);
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(yv[e]));
        }
    }
    if (A.xq == nullptr) return;  // only y was asked for
    RowDiv rd;
    rd.set(row_scale<MM>(amax, lane, A.xs + m));
    uint8_t* qrow = A.xq + m * N;
    int isum = 0;  // (quant8's row sum: unused here)
    for (int64_t p0 = 0; p0 < npass; p0 += U) {
        uint4 yp[U];
        if (lds) {
#pragma unroll
            for (int u = 0; u < U; ++u) yp[u] = img[(p0 + u < npass ? p0 + u : npass - 1) * 64 + lane];  // (inside the image; unused past the end)
        } else {
            compute(p0, yp);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t idx = (p0 + u) * 512 + lane * 8;
            float yv[8];
            Vec16<T_ID>::unpack(yp[u], yv);
            if (idx < N) store_codes8(qrow + idx, quant8<MM>(yv, rd, isum));
        }
    }
}

}  // namespace

extern "C" int sdnq_hip_act_rowquant(const void* a, const void* b, int x_dtype, int64_t m, int64_t n, int64_t lda, int64_t ldb, int act,
                                     int mm_dtype, void* y, void* xq, float* xs, sdnq_stream_t stream) {
    const int st = act_rowquant_check(a, b, x_dtype, m, n, lda, ldb, act, mm_dtype, y, xq, xs);
    if (st != SDNQ_OK) return st;
    ActQuantArgs A;
    A.a = a; A.b = b; A.M = m; A.N = n; A.lda = lda; A.ldb = ldb;
    A.y = y; A.xq = (uint8_t*)xq; A.xs = xs;
    A.pf = nullptr; A.pf_vecs = 0;
    const int np = (int)((n + 511) / 512);
    const bool reg = n <= ACT_REG_MAX_N;
    A.row_blocks = (int)(reg ? (m + 3) / 4 : m);  // four rows per workgroup | one
    A.use_lds = (!reg && xq && n <= ACT_LDS_MAX_N) ? 1 : 0;  // (nothing to hold for a y-only launch)
    const size_t lds_bytes = A.use_lds ? (size_t)np * 64 * sizeof(uint4) : 0;  // <= 32 KB
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)A.row_blocks), block(reg ? 256u : 64u);
#define AQ_REG(T, MMV, ACTV, G, NPV) hipLaunchKernelGGL((actquant_reg_kernel<T, MMV, ACTV, G, NPV>), grid, block, 0, s, A)
#define AQ_NP(T, MMV, ACTV, G)                                                                       \
    do {                                                                                             \
        if (!reg) hipLaunchKernelGGL((actquant_long_kernel<T, MMV, ACTV, G>), grid, block, lds_bytes, s, A); \
        else if (np <= 1) AQ_REG(T, MMV, ACTV, G, 1);                                                \
        else if (np <= 2) AQ_REG(T, MMV, ACTV, G, 2);                                                \
        else if (np <= 3) AQ_REG(T, MMV, ACTV, G, 3);                                                \
        else if (np <= 5) AQ_REG(T, MMV, ACTV, G, 5);                                                \
        else AQ_REG(T, MMV, ACTV, G, 8);                                                             \
    } while (0)
#define AQ_G(T, MMV, ACTV) do { if (b) AQ_NP(T, MMV, ACTV, true); else AQ_NP(T, MMV, ACTV, false); } while (0)
#define AQ_ACT(T, MMV)                                           \
    do {                                                         \
        if (act == ACT_GELU) AQ_G(T, MMV, ACT_GELU);             \
        else if (act == ACT_GELU_TANH) AQ_G(T, MMV, ACT_GELU_TANH); \
        else AQ_G(T, MMV, ACT_SILU);                             \
    } while (0)
#define AQ_MM(T) do { if (mm_dtype == SDNQ_MM_I8) AQ_ACT(T, SDNQ_MM_I8); else AQ_ACT(T, SDNQ_MM_FP8); } while (0)
    if (x_dtype == SDNQ_BF16) AQ_MM(SDNQ_BF16);
    else AQ_MM(SDNQ_F16);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
