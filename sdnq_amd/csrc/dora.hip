// DoRA (weight-decomposed LoRA, PEFT's use_dora) on frozen quantized Linear layers: the two passes that are new beside the adapter
// kernels of lowrank_train.hip.  No reference interface: the reference has no adapters; these replace what PEFT assembles around a
// quantized layer -- `torch.linalg.norm(dequantize(W) + scale * B @ A, dim=1)` (a float [N][K] weight, a second [N][K] product, an add,
// a square and a reduction) and, in the backward, `dY * mag_norm_scale` plus the row sums behind the gradient of the magnitude.
//
//   sdnq_hip_dora_normsq / _dense   out[n] = sum_k e^2, e = fmaf(scale, sum_r up[n][r] down[r][k], w32[n][k]), all in float32; w32 is
//       dequant16's value (weight_dev.h) of the stored codes, or for the _dense form load_row16's of a dense [N][K] operand.  The codes
//       are read once, nothing of size N x K is written.
//       A workgroup (4 waves) owns 16 rows n and walks K in chunks of DN_KC = 256: wave w takes the 64 columns 64 w .. of the chunk, and
//       its lane (li = lane % 16, g = lane / 16) the 16-run k0 = chunk + 64 w + 16 g of row n0 + li -- what dequant16 decodes.  The rank
//       product runs on v_mfma_f32_16x16x32 as C = down^T . up^T: B = 16 rows of up (read from global memory in fragment form, 16 bytes
//       per lane), A = 16 columns k of down, so that a lane's four accumulators of one MFMA are four consecutive k of ITS row: which 16
//       columns an MFMA takes is free, and tile j (0..3) takes k = 64 w + 16 a / 4 + 4 j + a % 4 for its row a -- lane (li, g) then holds
//       acc[j][e] = column 64 w + 16 g + 4 j + e, the element v[4 j + e] of its decoded run.  down [R][K] has the rank on the slow axis:
//       a rank step of 32 rows x 256 columns is staged in LDS as it lies in memory (16-byte chunks; rows past `rank`, columns past K as
//       zeros) and the A fragments -- 8 consecutive ranks of one column per lane -- come out by ds_read_b64_tr_b16, lane 4 q + p of a
//       16-lane group supplying rank row 8 g + q (and + 4), columns 64 w + 16 p + 4 j .. + 3.  EXEC is full at those reads: every
//       branch around them is workgroup-uniform, rows / runs outside the matrix are computed on zeros and discarded.
//       LDS rows of 528 bytes (512 + 16): a 32-lane half's transposed read is 2-way conflicted (worked out by hand, not measured), the
//       16-byte stores are aligned.  Two barriers per rank step; the global loads of a step (and of the codes) are issued before its first barrier.  Untuned
//       beyond that.
//       The order of the float32 sum is a constant of this file: a lane adds its 16 squares in ascending k by s = fmaf(e, e, s), chunk
//       after chunk; the 16 lane sums of a row are then added as ((p[0] + p[1]) + ...) in the order wave-major, g-minor.  One launch, no
//       atomics, no workspace, the same bits on every call, capturable.
//
//   sdnq_hip_dora_bwd   g = round_dtype(f32(dY) * c[n]) and q[n] = sum_i f32(dY[i][n]) * (f32(y[i][n]) - f32(bias[n])) in ONE pass over dY
//       (and y).  A workgroup takes a slab of DB_SLAB = 256 rows x 64 columns: thread t the 16-byte chunk t % 8 of rows t / 8 + 32 i,
//       i = 0..7, summed by fmaf in that order; the 32 thread sums of a column are added in ascending order through LDS.  One slab: the
//       workgroup stores q itself.  More: the slab sums go to workspace [slab][N] and a second launch adds them in ascending slab order --
//       the shape of sdnq_hip_lowrank_grad's reduction: no atomics, the same bits on every call.
#include "weight_dev.h"

namespace {

// (lowrank_dev.h has the same three; it also defines a kernel, which every unit that includes it carries a copy of)
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s* lds_v4s_ptr;

template <bool IS_BF16>
__device__ __forceinline__ v4f mfma16(v4i a, v4i b, v4f c) {
    if constexpr (IS_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

constexpr int DN_KC = 256;   // columns of K per workgroup iteration (64 per wave)
constexpr int DN_ROW = 528;  // bytes per LDS row of the staged rank step: 256 16-bit columns + 16
constexpr int DB_SLAB = 256; // rows of M per partial sum of sdnq_hip_dora_bwd (tests/dora_util.py restates it)

// DENSE: the weight operand is a dense [N][K] matrix of the factors' dtype (row stride ldw) instead of the stored codes of p
template <bool IS_BF16, bool DENSE>
__global__ __launch_bounds__(256) void dora_normsq_kernel(const DeqParams p, const uint16_t* __restrict__ wd, int64_t ldw,
                                                          const uint16_t* __restrict__ up, const uint16_t* __restrict__ down, int R,
                                                          float scale, float* __restrict__ out) {
    constexpr int T_ID = IS_BF16 ? SDNQ_BF16 : SDNQ_F16;
    __shared__ __attribute__((aligned(16))) uint8_t img[32 * DN_ROW];  // [rank of the step][k of the chunk]
    __shared__ float part[16][16];                                   // [4 wave + g][li]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15, q = (lane >> 2) & 3, pp = lane & 3;
    const int64_t n = (int64_t)blockIdx.x * 16 + li;
    const bool n_ok = n < p.N;
    const bool lowrank = up != nullptr;  // workgroup-uniform
    const v4i zero = {0, 0, 0, 0};
    float s = 0.0f;
    for (int64_t kb = 0; kb < p.K; kb += DN_KC) {
        const int64_t k0 = kb + 64 * wave + 16 * g;
        const bool run = n_ok && k0 < p.K;  // K % 16 == 0: a run of 16 never leaves its row
        float v[16];
        if (run) {
            if constexpr (DENSE) load_row16<T_ID>(wd, n * ldw + k0, v);
            else dequant16(p, n, k0, v);
        }
        v4f acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
        if (lowrank) {
            for (int rs = 0; rs < R; rs += 32) {
                // the step's global loads -- its four 16-byte chunks of down, its fragment of up -- go out before the barrier, beside the
                // loads of the codes: one memory latency per step instead of three in a row
                v4i d[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = tid + 256 * i, r = o >> 5, ch = o & 31;
                    const int64_t kk = kb + 8 * ch;
                    d[i] = (rs + r < R && kk < p.K) ? *(const v4i*)(down + (int64_t)(rs + r) * p.K + kk) : zero;
                }
                const int rc = rs + 8 * g;  // rank % 8 == 0: a chunk is inside the row of up or past it
                const v4i fb = (n_ok && rc < R) ? *(const v4i*)(up + n * R + rc) : zero;
                __syncthreads();  // the reads of the step before are done
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = tid + 256 * i, r = o >> 5, ch = o & 31;
                    *(v4i*)(img + r * DN_ROW + 16 * ch) = d[i];
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t* a0 = img + (8 * g + q) * DN_ROW + 2 * (64 * wave + 16 * pp + 4 * j);
                    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_ptr)a0);
                    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_ptr)(a0 + 4 * DN_ROW));
                    const v2i l2 = __builtin_bit_cast(v2i, lo), h2 = __builtin_bit_cast(v2i, hi);
                    acc[j] = mfma16<IS_BF16>((v4i){l2[0], l2[1], h2[0], h2[1]}, fb, acc[j]);
                }
            }
        }
        if (run) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = lowrank ? fmaf(scale, acc[j][e], v[4 * j + e]) : v[4 * j + e];
                    s = fmaf(x, x, s);
                }
        }
    }
    part[4 * wave + g][li] = s;
    __syncthreads();
    if (tid < 16) {
        const int64_t no = (int64_t)blockIdx.x * 16 + tid;
        if (no < p.N) {
            float t = part[0][tid];
#pragma unroll
            for (int i = 1; i < 16; ++i) t += part[i][tid];
            out[no] = t;
        }
    }
}

template <int T_ID, bool HAS_Q>
__global__ __launch_bounds__(256) void dora_bwd_kernel(const uint16_t* __restrict__ dy, int64_t lddy, const uint16_t* __restrict__ y, int64_t ldy,
                                                       const uint16_t* __restrict__ bias, const float* __restrict__ c, int64_t M, int64_t N,
                                                       uint16_t* __restrict__ gout, float* __restrict__ dst) {
    __shared__ float red[32][65];
    const int tid = threadIdx.x, cc = tid & 7, rl = tid >> 3;
    const int64_t n = (int64_t)blockIdx.x * 64 + 8 * cc, m0 = (int64_t)blockIdx.y * DB_SLAB;
    const bool n_ok = n < N;  // N % 8 == 0: the 8 columns are inside the row or past it
    float cv[8], bv[8], acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { cv[e] = 0.0f; bv[e] = 0.0f; acc[e] = 0.0f; }
    if (n_ok) {
        Vec16<SDNQ_F32>::unpack(*(const uint4*)(c + n), cv);
        Vec16<SDNQ_F32>::unpack(*(const uint4*)(c + n + 4), cv + 4);
        if (HAS_Q && bias) Vec16<T_ID>::unpack(*(const uint4*)(bias + n), bv);
    }
#pragma unroll
    for (int i = 0; i < DB_SLAB / 32; ++i) {
        const int64_t m = m0 + rl + 32 * i;
        if (n_ok && m < M) {
            float f[8], o[8];
            Vec16<T_ID>::unpack(*(const uint4*)(dy + m * lddy + n), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f[e] * cv[e];
            *(uint4*)(gout + m * N + n) = Vec16<T_ID>::pack(o);
            if constexpr (HAS_Q) {
                float yv[8];
                Vec16<T_ID>::unpack(*(const uint4*)(y + m * ldy + n), yv);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(f[e], yv[e] - bv[e], acc[e]);
            }
        }
    }
    if constexpr (HAS_Q) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[rl][8 * cc + e] = acc[e];
        __syncthreads();
        if (tid < 64) {
            const int64_t no = (int64_t)blockIdx.x * 64 + tid;
            if (no < N) {
                float t = red[0][tid];
#pragma unroll
                for (int r = 1; r < 32; ++r) t += red[r][tid];
                dst[(int64_t)blockIdx.y * N + no] = t;
            }
        }
    }
}

// q[n] = ((part[0][n] + part[1][n]) + part[2][n]) + ...: one thread per column, slabs in ascending order
__global__ __launch_bounds__(256) void dora_bwd_sum_kernel(const float* __restrict__ part, int64_t slabs, int64_t N, float* __restrict__ q) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = part[n];
    for (int64_t k = 1; k < slabs; ++k) s += part[k * N + n];
    q[n] = s;
}

// the checks and the launch both norm entry points share; p holds N and K (and, for the codes, everything dequant16 reads)
int dora_normsq_launch(const DeqParams& p, const void* wd, int64_t ldw, const void* up, const void* down, int dtype, int rank, float scale,
                       float* out, sdnq_stream_t stream) {
    if (!out) return SDNQ_ERR_NULL;
    if ((up == nullptr) != (down == nullptr)) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if ((p.K % 16) != 0 || (p.N % 8) != 0) return SDNQ_ERR_SHAPE;
    if (up && (rank < 8 || rank > 256 || (rank % 8) != 0)) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)up % 16) || ((uintptr_t)down % 16) || ((uintptr_t)out % 4)) return SDNQ_ERR_ALIGN;
    const int64_t gx = (p.N + 15) / 16;
    if (gx > 0x7fffffff) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx), block(256);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, p, (const uint16_t*)wd, ldw, (const uint16_t*)up, (const uint16_t*)down, rank, scale, out);
    };
    if (wd) { if (dtype == SDNQ_BF16) launch(dora_normsq_kernel<true, true>); else launch(dora_normsq_kernel<false, true>); }
    else { if (dtype == SDNQ_BF16) launch(dora_normsq_kernel<true, false>); else launch(dora_normsq_kernel<false, false>); }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

}  // namespace

extern "C" int sdnq_hip_dora_normsq(const SdnqWeight* w, const void* up, const void* down, int dtype, int rank, float scale, float* out,
                                    sdnq_stream_t stream) {
    DeqParams p{};
    const int st = fill_params(w, p);  // NULL, formats, group shape, K % 16, code alignment
    if (st != SDNQ_OK) return st;
    if (p.svd_up) return SDNQ_ERR_UNSUPPORTED;  // the SVD product is not fused: sdnq_hip_dequant + sdnq_hip_dora_normsq_dense
    return dora_normsq_launch(p, nullptr, 0, up, down, dtype, rank, scale, out, stream);
}

extern "C" int sdnq_hip_dora_normsq_dense(const void* wd, int dtype, int64_t n, int64_t k, int64_t ldw, const void* up, const void* down,
                                          int rank, float scale, float* out, sdnq_stream_t stream) {
    if (!wd) return SDNQ_ERR_NULL;
    if (n <= 0 || k <= 0 || ldw < k) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)wd % 16) || ((ldw * 2) % 16)) return SDNQ_ERR_ALIGN;
    DeqParams p{};
    p.N = n; p.K = k;
    return dora_normsq_launch(p, wd, ldw, up, down, dtype, rank, scale, out, stream);
}

extern "C" int64_t sdnq_hip_dora_bwd_workspace_bytes(int64_t m, int64_t n) {
    if (m <= 0 || n <= 0 || (n % 8) != 0) return SDNQ_ERR_SHAPE;
    const int64_t slabs = (m + DB_SLAB - 1) / DB_SLAB;
    return slabs <= 1 ? 0 : slabs * n * 4;
}

extern "C" int sdnq_hip_dora_bwd(const void* dy, int64_t lddy, const void* y, int64_t ldy, const void* bias, const float* c, int dtype,
                                 int64_t m, int64_t n, void* g, float* q, void* workspace, int64_t workspace_bytes, sdnq_stream_t stream) {
    if (!dy || !c || !g || (q && !y)) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (m <= 0 || n <= 0 || (n % 8) != 0 || lddy < n || (q && ldy < n)) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)dy % 16) || ((lddy * 2) % 16) || ((uintptr_t)g % 16) || ((uintptr_t)c % 16) || ((uintptr_t)bias % 16)) return SDNQ_ERR_ALIGN;
    if (q && (((uintptr_t)y % 16) || ((ldy * 2) % 16) || ((uintptr_t)q % 4))) return SDNQ_ERR_ALIGN;
    const int64_t slabs = (m + DB_SLAB - 1) / DB_SLAB;
    const int64_t need = q ? sdnq_hip_dora_bwd_workspace_bytes(m, n) : 0;
    if (need > 0) {
        if (!workspace) return SDNQ_ERR_NULL;
        if (workspace_bytes < need) return SDNQ_ERR_SHAPE;
        if ((uintptr_t)workspace % 16) return SDNQ_ERR_ALIGN;
    }
    const int64_t gx = (n + 63) / 64;
    if (gx > 0x7fffffff || slabs > 65535 || (n + 255) / 256 > 0x7fffffff) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)slabs), block(256);
    hipStream_t s = (hipStream_t)stream;
    float* dst = need > 0 ? (float*)workspace : q;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)dy, lddy, (const uint16_t*)y, ldy, (const uint16_t*)bias, c, m, n,
                           (uint16_t*)g, dst);
    };
    if (dtype == SDNQ_BF16) { if (q) launch(dora_bwd_kernel<SDNQ_BF16, true>); else launch(dora_bwd_kernel<SDNQ_BF16, false>); }
    else { if (q) launch(dora_bwd_kernel<SDNQ_F16, true>); else launch(dora_bwd_kernel<SDNQ_F16, false>); }
    SDNQ_CHECK_LAUNCH();
    if (need > 0) {
        hipLaunchKernelGGL(dora_bwd_sum_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, s, (const float*)workspace, slabs, n, q);
        SDNQ_CHECK_LAUNCH();
    }
    return SDNQ_OK;
}
