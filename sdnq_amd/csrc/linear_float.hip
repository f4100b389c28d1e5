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
template <bool IS_BF16, int RT>
__global__ __launch_bounds__(256) void lowrank_down_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ down,
                                                           uint16_t* __restrict__ t, int64_t M, int64_t K, int64_t ldx, int R) {
    SDNQ_KERNARGS_NOW("s"(x), "s"(down), "s"(t), "s"(M), "s"(K), "s"(ldx), "s"(R));
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int NS = 4, XS = RT * 16 * 256, STAGE = XS + 32 * 256;  // 12 / 16 KB per stage; 48 / 64 KB ring
    constexpr int NDMA = RT + 2;  // DMAs per wave and stage
    __shared__ __attribute__((aligned(1024))) uint8_t lds[NS * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * (16 * RT);
    const int n_tiles = (R + 31) / 32;
    const int64_t nst = (K + 127) / 128;
    // DMA role of this lane: row 4 * wave + lane / 16 of every activation tile and of each half of the factor tile; physical chunk
    // lane % 16 holds logical chunk (lane % 16) ^ row
    const int drow = wave * 4 + (lane >> 4);
    const int lchunk = (lane & 15) ^ drow;
    // fragment role: row lane & 15, logical chunk 4 * wave + lane / 16 of the stage
    const int frow = lane & 15;
    const int foff = frow * 256 + (((wave * 4 + (lane >> 4)) ^ frow) << 4);
    const uint16_t* sx[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        int64_t gm = m0 + r * 16 + drow;
        if (gm >= M) gm = M - 1;
        sx[r] = x + gm * ldx + lchunk * 8;
    }
    for (int nt = 0; nt < n_tiles; ++nt) {
        const int gn0 = nt * 32 + drow, gn1 = gn0 + 16;
        const uint16_t* sd0 = down + (int64_t)(gn0 < R ? gn0 : 0) * K + lchunk * 8;  // rows past R: valid memory, never stored
        const uint16_t* sd1 = down + (int64_t)(gn1 < R ? gn1 : 0) * K + lchunk * 8;
        auto issue = [&](int64_t st) {  // stages past the end of K are all-zero DMAs: the counted vmcnt stays a constant
            uint8_t* base = lds + (st % NS) * STAGE;
            const int64_t k0 = st * 128;
            const bool ok = k0 + lchunk * 8 < K;
            const uintptr_t z = (uintptr_t)&g_lr_zero16;  // (integer selects: a pointer ternary became three divergent branches)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const uintptr_t px = ok ? (uintptr_t)(sx[r] + k0) : z;
                __builtin_amdgcn_global_load_lds((gptr_t)px, (lptr_t)(base + r * 4096 + wave * 1024), 16, 0, 0);
            }
            const uintptr_t p0 = ok ? (uintptr_t)(sd0 + k0) : z, p1 = ok ? (uintptr_t)(sd1 + k0) : z;
            __builtin_amdgcn_global_load_lds((gptr_t)p0, (lptr_t)(base + XS + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)p1, (lptr_t)(base + XS + 4096 + wave * 1024), 16, 0, 0);
        };
        v4f acc[RT][2];
#pragma unroll
        for (int r = 0; r < RT; ++r) { acc[r][0] = (v4f){0.0f, 0.0f, 0.0f, 0.0f}; acc[r][1] = (v4f){0.0f, 0.0f, 0.0f, 0.0f}; }
#pragma unroll
        for (int s0 = 0; s0 < NS - 1; ++s0) issue(s0);
        for (int64_t st = 0; st < nst; ++st) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * NDMA) : "memory");  // this wave's pieces of stage st have landed
            // ... and everybody's; every wave is also done reading stage st - 1 (its fragments fed MFMAs already), whose slot is
            // refilled next.  Raw s_barrier: __syncthreads() would drain the DMAs in flight (s_waitcnt vmcnt(0)).
            __builtin_amdgcn_s_barrier();
            issue(st + NS - 1);
            const uint8_t* base = lds + (st % NS) * STAGE;
            // (ext-vector loads: an LDS read typed as the HIP uint4 struct makes the compiler drain the LDS-DMAs first, vmcnt(0))
            v4i fx[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) fx[r] = *(const v4i*)(base + r * 4096 + foff);
            const v4i f0 = *(const v4i*)(base + XS + foff);
            const v4i f1 = *(const v4i*)(base + XS + 4096 + foff);
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                if constexpr (IS_BF16) {
                    acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, f0), __builtin_bit_cast(v8bf, fx[r]), acc[r][0], 0, 0, 0);
                    acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, f1), __builtin_bit_cast(v8bf, fx[r]), acc[r][1], 0, 0, 0);
                } else {
                    acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, f0), __builtin_bit_cast(v8h, fx[r]), acc[r][0], 0, 0, 0);
                    acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, f1), __builtin_bit_cast(v8h, fx[r]), acc[r][1], 0, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing zero DMAs target the ring the partial sums reuse
        __syncthreads();
        float* part = (float*)lds;  // [4 waves][RT row tiles][2 rank halves][4 regs][64 lanes]
        constexpr int WSTRIDE = RT * 2 * 4 * 64;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) part[wave * WSTRIDE + ((r * 2 + h) * 4 + e) * 64 + lane] = acc[r][h][e];
        __syncthreads();
        // accumulator layout: lane l of (row tile r, rank half h) holds n = 16 h + 4 (l >> 4) + e, m = 16 r + (l & 15).  Consecutive
        // threads take consecutive n of one row (64-byte runs of t)
#pragma unroll
        for (int o = tid; o < RT * 512; o += 256) {
            const int n = o & 31, m = o >> 5;
            const int r = m >> 4, ml = m & 15, h = n >> 4, q = n & 15, l = (q >> 2) * 16 + ml, e = q & 3;
            const int idx = ((r * 2 + h) * 4 + e) * 64 + l;
            const float sum = (part[idx] + part[WSTRIDE + idx]) + (part[2 * WSTRIDE + idx] + part[3 * WSTRIDE + idx]);
            const int gn = nt * 32 + n;
            if (m0 + m < M && gn < R) t[(m0 + m) * R + gn] = IS_BF16 ? f32_to_bf16_bits(sum) : f32_to_f16_bits(sum);
        }
        __syncthreads();  // partial sums consumed before the next n-tile's DMAs overwrite them
    }
}

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

extern "C" int sdnq_hip_lowrank_down(const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, const void* svd_down,
                                     int svd_dtype, int rank, void* t, sdnq_stream_t stream) {
    // t = mm(x.to(svd dtype), svd_down): x already lives in the activation dtype; the reference casts x to
    // svd_down.dtype first (linear_int8.py:60) -- both are the model dtype, so require equality.
    if (x_dtype != svd_dtype) return SDNQ_ERR_DTYPE;
    if (x_dtype != SDNQ_F32 && (k % 16) == 0 && rank > 0 && x && svd_down && t && ((uintptr_t)x % 16) == 0 &&
        ((uintptr_t)svd_down % 16) == 0 && ((ldx * 2) % 16) == 0) {
        hipStream_t s = (hipStream_t)stream;
        // row tiles per workgroup: whichever leaves the busiest CU fewer bytes to move (see the kernel; 3 : 4 = bytes per workgroup and stage)
        static const int rt_env = [] { const char* e = getenv("SDNQ_HIP_LRD_RT"); return e ? atoi(e) : 0; }();  // tuning aid: 1 / 2
        const int64_t wg1 = (m + 15) / 16, wg2 = (m + 31) / 32;
        const int64_t cus = 256;
        const bool two = rt_env ? rt_env == 2 : ((wg2 + cus - 1) / cus) * 4 < ((wg1 + cus - 1) / cus) * 3;
        dim3 grid((unsigned)(two ? wg2 : wg1)), block(256);
        auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)svd_down, (uint16_t*)t, m, k, ldx, rank); };
        if (x_dtype == SDNQ_BF16) launch(two ? lowrank_down_kernel<true, 2> : lowrank_down_kernel<true, 1>);
        else launch(two ? lowrank_down_kernel<false, 2> : lowrank_down_kernel<false, 1>);
        SDNQ_CHECK_LAUNCH();
        return SDNQ_OK;
    }
    return sdnq_hip_linear_float(x, svd_down, nullptr, x_dtype, t, m, rank, k, ldx, stream);
}
