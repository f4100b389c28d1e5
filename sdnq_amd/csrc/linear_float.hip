// Float linears for gfx950: the kernels that never see an SdnqWeight.
//
//   sdnq_hip_linear_float(_strided) <- torch.nn.functional.linear on the dequantized weight
//                                      (layers/linear/forward.py:25-26; M<32 branch linear_int8.py:102-103): linear_float_kernel for a
//                                      few rows, the MFMA GEMM of gemm.hip (sdnq_float_gemm) beyond 32
//   sdnq_hip_linear_float_f32out(_strided) <- the same product with the float32 accumulators stored unrounded and no bias: the `cols`
//                                      of a transposed convolution (convt.hip), rounded once after the taps are added
//   sdnq_hip_lowrank_down           <- t = torch.mm(x, svd_down), the inner product of the SVD branch (linear_int8.py:60):
//                                      lowrank_down_kernel on the matrix cores, linear_float_kernel for float32
#include "gemm_dev.h"  // sdnq_float_gemm
#include "philox_dev.h"  // dropout_chunk: the mask of sdnq_hip_lowrank_down_dropout

namespace {

// out[m][n] = cast( sum_k x[m][k] * w[n][k] + bias[n] ), fp32 accumulate.
// One wave per output channel n and a chunk of MC activation rows; lanes stride K in 16-byte vectors.
// O_ID: the output element type (T_ID; SDNQ_F32 for the float32 store of sdnq_hip_linear_float_f32out).
template <int T_ID, int MC, int O_ID = T_ID>
__global__ __launch_bounds__(256) void linear_float_kernel(const void* __restrict__ x, const void* __restrict__ w,
                                                           const void* __restrict__ bias, void* __restrict__ out, int64_t M,
                                                           int64_t N, int64_t K, int64_t ldx, int64_t ldc) {
    constexpr int VN = Vec16<T_ID>::n;
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t m0 = (int64_t)blockIdx.y * MC;
    if (n >= N) return;
    float acc[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) acc[i] = 0.0f;
    const uint8_t* wrow = (const uint8_t*)w + n * K * FT<T_ID>::bytes;
    for (int64_t k = (int64_t)lane * VN; k < K; k += 64 * VN) {
        float wv[VN];
        Vec16<T_ID>::unpack(*(const uint4*)(wrow + k * FT<T_ID>::bytes), wv);
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const int64_t m = (m0 + i < M) ? m0 + i : M - 1;
            float xv[VN];
            Vec16<T_ID>::unpack(*(const uint4*)((const uint8_t*)x + (m * ldx + k) * FT<T_ID>::bytes), xv);
#pragma unroll
            for (int e = 0; e < VN; ++e) acc[i] = fmaf(xv[e], wv[e], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        float s = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0 && m0 + i < M) {
            if (bias) s += FT<T_ID>::load(bias, n);
            FT<O_ID>::store(out, (m0 + i) * ldc + n, s);
        }
    }
}

// t[M][R] = cast( x[M][K] . down[R][K]^T ) on the matrix cores (bf16 / f16): the inner torch.mm of the SVD branch
// (linear_int8.py:60).  HBM-bound on x: 2*M*K bytes (28 MB for a FLUX activation).
// One workgroup (4 waves) = 16 activation rows x all of K x 32 factor rows, walked in stages of 128 k through an LDS ring:
//   HBM / L2 -> LDS by LDS-DMA (global_load_lds_dwordx4: no registers, so the ring depth -- not the compiler's s_waitcnt model --
//   decides how many stages are in flight): a piece = 4 rows x 256 bytes, lane l -> row l / 16, 16-byte chunk l % 16, XOR-swizzled
//   on the global side so that LDS stays lane-linear; 4 activation + 8 factor pieces per stage, 3 per wave;
//   LDS -> v_mfma_f32_16x16x32 fragments: wave w owns k-step w of every stage (A = factor rows, B = activation rows); the 16 rows of
//   a fragment read hit 16 different bank groups thanks to the swizzle.
// History (rounds 1-2): the fragments used to be loaded straight from global memory in the MFMA layout -- lane l = row (l & 15) at
// a 6 KB row stride = 64 different cache lines per load instruction -- and the L1 tag rate, not HBM, bounded the kernel: 20-24 us
// per call at 4608 x 3072 whatever the software pipelining, 12 us even for 77 rows.  A register-staged coalesced variant lost to
// the compiler's pessimistic s_waitcnt on loop-carried loads (47 us).
__device__ const uint4 g_lr_zero16 = {0u, 0u, 0u, 0u};  // source of chunks past the end of K
// RT = activation row tiles of 16 per workgroup.  What bounds the kernel is the LDS-DMA rate of a CU (a stage moves 4 KB of activations
// per row tile and ALWAYS 8 KB of factor rows), so the launcher picks RT by the largest number of bytes a CU has to move: 4608 rows are
// 288 workgroups of one tile -- 32 CUs get two, 2 x 288 KB per K = 3072 -- or 144 workgroups of two tiles, 384 KB each: 8.5 -> 6 us.
// The kernel's text lives in lowrank_down_kernel.h, included once per form: lowrank_down_kernel<IS_BF16, RT> and
// lowrank_down_dropout_kernel<IS_BF16, RT> (sdnq_hip_lowrank_down_dropout).
#define LR_DROP 0
#include "lowrank_down_kernel.h"
#undef LR_DROP
#define LR_DROP 1
#include "lowrank_down_kernel.h"
#undef LR_DROP

}  // namespace

extern "C" int sdnq_hip_linear_float_strided(const void* x, const void* wd, const void* bias, int dtype, void* out, int64_t m,
                                             int64_t n, int64_t k, int64_t ldx, int64_t ldc, sdnq_stream_t stream) {
    if (!x || !wd || !out) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    const int eb = (dtype == SDNQ_F32) ? 4 : 2;
    if (m <= 0 || n <= 0 || k <= 0 || ldx < k || ldc < n || ((k * eb) % 16) != 0) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((uintptr_t)wd % 16) || ((ldx * eb) % 16)) return SDNQ_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    // more than a few rows: the MFMA GEMM of gemm.hip (bf16 / f16 / f32 matrix cores); its stores are 8 channels wide
    if (m > 32 && (n % 8) == 0 && ((uintptr_t)out % 16) == 0 && ((ldc * eb) % 16) == 0)
        return sdnq_float_gemm(x, wd, bias, dtype, out, m, n, k, ldx, s, nullptr, 0, 0, ldc);
    constexpr int MC = 8;
    dim3 grid((unsigned)((n + 3) / 4), (unsigned)((m + MC - 1) / MC)), block(256);
    switch (dtype) {
        case SDNQ_F32: hipLaunchKernelGGL((linear_float_kernel<SDNQ_F32, MC>), grid, block, 0, s, x, wd, bias, out, m, n, k, ldx, ldc); break;
        case SDNQ_BF16: hipLaunchKernelGGL((linear_float_kernel<SDNQ_BF16, MC>), grid, block, 0, s, x, wd, bias, out, m, n, k, ldx, ldc); break;
        default: hipLaunchKernelGGL((linear_float_kernel<SDNQ_F16, MC>), grid, block, 0, s, x, wd, bias, out, m, n, k, ldx, ldc); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_linear_float(const void* x, const void* wd, const void* bias, int dtype, void* out, int64_t m,
                                     int64_t n, int64_t k, int64_t ldx, sdnq_stream_t stream) {
    return sdnq_hip_linear_float_strided(x, wd, bias, dtype, out, m, n, k, ldx, n, stream);
}

extern "C" int sdnq_hip_linear_float_f32out_strided(const void* x, const void* wd, int dtype, float* out, int64_t m, int64_t n, int64_t k,
                                                    int64_t ldx, int64_t ldc, sdnq_stream_t stream) {
    if (!x || !wd || !out) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    const int eb = (dtype == SDNQ_F32) ? 4 : 2;
    if (m <= 0 || n <= 0 || k <= 0 || ldx < k || ldc < n || ((k * eb) % 16) != 0) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((uintptr_t)wd % 16) || ((ldx * eb) % 16) || ((uintptr_t)out % 4)) return SDNQ_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (m > 32 && (n % 8) == 0 && ((uintptr_t)out % 16) == 0 && ((ldc * 4) % 16) == 0)
        return sdnq_float_gemm_f32out(x, wd, dtype, out, m, n, k, ldx, ldc, s);
    constexpr int MC = 8;
    dim3 grid((unsigned)((n + 3) / 4), (unsigned)((m + MC - 1) / MC)), block(256);
    const void* nobias = nullptr;
    switch (dtype) {
        case SDNQ_F32: hipLaunchKernelGGL((linear_float_kernel<SDNQ_F32, MC>), grid, block, 0, s, x, wd, nobias, (void*)out, m, n, k, ldx, ldc); break;
        case SDNQ_BF16: hipLaunchKernelGGL((linear_float_kernel<SDNQ_BF16, MC, SDNQ_F32>), grid, block, 0, s, x, wd, nobias, (void*)out, m, n, k, ldx, ldc); break;
        default: hipLaunchKernelGGL((linear_float_kernel<SDNQ_F16, MC, SDNQ_F32>), grid, block, 0, s, x, wd, nobias, (void*)out, m, n, k, ldx, ldc); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_linear_float_f32out(const void* x, const void* wd, int dtype, float* out, int64_t m, int64_t n, int64_t k,
                                            int64_t ldx, sdnq_stream_t stream) {
    return sdnq_hip_linear_float_f32out_strided(x, wd, dtype, out, m, n, k, ldx, n, stream);
}

// row tiles per workgroup of lowrank_down_kernel: whichever leaves the busiest CU fewer bytes to move (see the kernel; 3 : 4 = bytes per
// workgroup and stage)
static bool lowrank_down_two_tiles(int64_t m) {
    static const int rt_env = [] { const char* e = getenv("SDNQ_HIP_LRD_RT"); return e ? atoi(e) : 0; }();  // tuning aid: 1 / 2
    const int64_t wg1 = (m + 15) / 16, wg2 = (m + 31) / 32;
    const int64_t cus = 256;
    return rt_env ? rt_env == 2 : ((wg2 + cus - 1) / cus) * 4 < ((wg1 + cus - 1) / cus) * 3;
}

extern "C" int sdnq_hip_lowrank_down(const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, const void* svd_down,
                                     int svd_dtype, int rank, void* t, sdnq_stream_t stream) {
    // t = mm(x.to(svd dtype), svd_down): x already lives in the activation dtype; the reference casts x to
    // svd_down.dtype first (linear_int8.py:60) -- both are the model dtype, so require equality.
    if (x_dtype != svd_dtype) return SDNQ_ERR_DTYPE;
    if (x_dtype != SDNQ_F32 && (k % 16) == 0 && rank > 0 && x && svd_down && t && ((uintptr_t)x % 16) == 0 &&
        ((uintptr_t)svd_down % 16) == 0 && ((ldx * 2) % 16) == 0) {
        hipStream_t s = (hipStream_t)stream;
        const bool two = lowrank_down_two_tiles(m);
        dim3 grid((unsigned)(two ? (m + 31) / 32 : (m + 15) / 16)), block(256);
        auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)svd_down, (uint16_t*)t, m, k, ldx, rank); };
        if (x_dtype == SDNQ_BF16) launch(two ? lowrank_down_kernel<true, 2> : lowrank_down_kernel<true, 1>);
        else launch(two ? lowrank_down_kernel<false, 2> : lowrank_down_kernel<false, 1>);
        SDNQ_CHECK_LAUNCH();
        return SDNQ_OK;
    }
    return sdnq_hip_linear_float(x, svd_down, nullptr, x_dtype, t, m, rank, k, ldx, stream);
}

extern "C" int sdnq_hip_lowrank_down_dropout(const void* x, int dtype, int64_t m, int64_t k, int64_t ldx, const void* down, int rank,
                                             void* t, int threshold, uint64_t seed, uint64_t offset, sdnq_stream_t stream) {
    // the matrix-core kernel only: no float32 and no few-row fallback (16 | K)
    if (!x || !down || !t) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (m <= 0 || k <= 0 || (k % 16) != 0 || ldx < k || rank <= 0 || threshold < 1 || threshold > 65535) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((uintptr_t)down % 16) || ((ldx * 2) % 16)) return SDNQ_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const bool two = lowrank_down_two_tiles(m);
    const int64_t wgs = two ? (m + 31) / 32 : (m + 15) / 16;
    if (wgs > 0x7fffffff) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)wgs), block(256);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)down, (uint16_t*)t, m, k, ldx, rank, (u32)threshold,
                           (u32)seed, (u32)(seed >> 32), (u32)offset, (u32)(offset >> 32));
    };
    if (dtype == SDNQ_BF16) launch(two ? lowrank_down_dropout_kernel<true, 2> : lowrank_down_dropout_kernel<true, 1>);
    else launch(two ? lowrank_down_dropout_kernel<false, 2> : lowrank_down_dropout_kernel<false, 1>);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
