// Few-row linears on stored codes for gfx950: y = x . dequant(W)^T + b for M of a few rows, where the weight is read once, as
// stored, and never exists dequantized in memory (the M < 32 branch of the quantized Linear, linear_int8.py:102-103).
//
//   sdnq_hip_linear_skinny     <- dequantize_weight (dequantizer.py:15-87, Hadamard :82-87) + torch.nn.functional.linear:
//                                 linear_skinny_kernel (every storage format, M <= 64), linear_skinny_fast_kernel (int8 / int4
//                                 codes, M <= 4), linear_skinny_had256_kernel (the same with Hadamard group 256 on the matrix cores)
//   sdnq_hip_linear_skinny_svd <- the same on a weight with SVD factors (dequantizer.py:79-83): skinny_svd_kernel, and
//                                 skinny_svd32_kernel for rank 32
//
// Latency-bound kernels, each tuned on its own: their code-to-float decodes and load schedules differ on purpose.
#include "hadamard_dev.h"
#include "weight_dev.h"

namespace {

// Fused skinny linear (M < 32): out[m][n] = cast( sum_k x[m][k] * round_T(dequant(W)[n][k]) + bias[n] ).
// Streams the QUANTIZED weight exactly once (bits/8 bytes per element instead of writing and re-reading a 2-byte
// dequantized copy): one wave per output channel, a lane decodes 16 consecutive elements per pass with the same
// arithmetic as sdnq_hip_dequant (f32(w)*s | fma, one rounding to the activation dtype T -- the reference rounds the
// dequantized weight to result_dtype before F.linear, dequantizer.py:82-83), fp32 accumulate, wave reduction.
// MROWS activation rows per launch column (grid.y walks M); x slices are re-read per channel from L1/L2.
// log2had != 0: the stored weight is Hadamard-rotated; the rounded dequantized run is un-rotated in registers (FWHT across
// the wave, 1024 elements per pass, groups never straddle a pass) and rounded to T again, exactly the order of the
// reference (dequantize -> .to(result_dtype) -> rotate_hadamard in result_dtype, dequantizer.py:82-87).
template <int T_ID, int MROWS>
__global__ __launch_bounds__(256) void linear_skinny_kernel(const DeqParams p, const void* __restrict__ x, const void* __restrict__ bias,
                                                            void* __restrict__ out, int64_t M, int64_t ldx, int log2had) {
    SDNQ_DEQ_ARGS_NOW(p);
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t m0 = (int64_t)blockIdx.y * MROWS;
    if (n >= p.N) return;
    float acc[MROWS];
#pragma unroll
    for (int i = 0; i < MROWS; ++i) acc[i] = 0.0f;
    const float hscale = log2had ? hadamard_scale(log2had, T_ID) : 1.0f;
    for (int64_t kb = 0; kb < p.K; kb += 1024) {  // wave-uniform trip count: the FWHT shuffles need every lane
        const int64_t k0 = kb + (int64_t)lane * 16;
        const bool live = k0 < p.K;
        float w[16];
        if (live) {
            dequant16(p, n, k0, w);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = FT<T_ID>::round(w[j]);
        if (log2had) {
            wave_hadamard16(w, log2had, hscale);
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = FT<T_ID>::round(w[j]);
        }
        if (!live) continue;
#pragma unroll
        for (int i = 0; i < MROWS; ++i) {
            const int64_t m = (m0 + i < M) ? m0 + i : M - 1;
            float xv[16];
            load_row16<T_ID>(x, m * ldx + k0, xv);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[i] = fmaf(xv[j], w[j], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < MROWS; ++i) {
        float sum = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0 && m0 + i < M) {
            if (bias) sum += FT<T_ID>::load(bias, n);
            FT<T_ID>::store(out, (m0 + i) * p.N + n, sum);
        }
    }
}

// Fast few-row linear for the two storage formats that matter at M <= 4 (raw 8-bit integers and 4-bit packed integers, signed
// or unsigned, any group size that is a multiple of 16): the generic kernel above decodes inside its K loop, so a wave has ONE
// 0.5-1 KiB weight load in flight and runs at 0.7-1.2 TB/s; here the loads of up to four 1024-element chunks of the row are
// issued before anything is decoded (3-4 KiB in flight per wave, ~20 waves per CU), everything else -- f32(w)*s | fma, rounding
// to T, optional FWHT un-rotation, fp32 accumulation, wave reduction -- is the same arithmetic in the same order.
template <int T_ID, int BITS, int MROWS>
__global__ __launch_bounds__(256) void linear_skinny_fast_kernel(const DeqParams p, const void* __restrict__ x, const void* __restrict__ bias,
                                                                 void* __restrict__ out, int64_t M, int64_t ldx, int log2had) {
    SDNQ_DEQ_ARGS_NOW(p);
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= p.N) return;
    float acc[MROWS];
#pragma unroll
    for (int i = 0; i < MROWS; ++i) acc[i] = 0.0f;
    const float hscale = log2had ? hadamard_scale(log2had, T_ID) : 1.0f;
    const uint8_t* wrow = (const uint8_t*)p.w + (BITS == 8 ? n * p.K : n * p.K / 2);
    const float* srow = p.scale + n * p.G;
    const float* zrow = p.zp ? p.zp + n * p.G : nullptr;
    const bool is_signed = p.fmt.kind == SDNQ_KIND_INT;
    constexpr bool PFX = MROWS == 1 && T_ID != SDNQ_F32;  // single activation row: its pieces are fetched with the weights
    for (int64_t kb = 0; kb < p.K; kb += 4096) {
        // every load of this 4096-element stretch first -- codes, scales / zero points, (one-row case) activations -- all
        // UNCONDITIONAL with clamped addresses: a load under a per-lane condition gets its own s_waitcnt vmcnt(0), and a scale
        // fetched next to its use adds a dependent round trip per chunk (round 2: 45 us for FLUX's 18432 x 3072 int4 layers, 7 us of
        // weight traffic)
        uint4 raw[4], xr[PFX ? 4 : 1][2];
        float scv[4], zpv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t k0 = kb + c * 1024 + (int64_t)lane * 16;
            const int64_t ks = k0 < p.K ? k0 : 0;
            if constexpr (BITS == 8) raw[c] = *(const uint4*)(wrow + ks);
            else { const uint2 q = *(const uint2*)(wrow + ks / 2); raw[c] = make_uint4(q.x, q.y, 0, 0); }
            const int g = (int)(ks / p.group_size);  // group_size % 16 == 0: one group per 16-run
            scv[c] = srow[g];
            zpv[c] = zrow ? zrow[g] : 0.0f;
            if constexpr (PFX) {
                xr[c][0] = *(const uint4*)((const uint16_t*)x + ks);
                xr[c][1] = *(const uint4*)((const uint16_t*)x + ks + 8);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (kb + c * 1024 >= p.K) break;  // wave-uniform
            const int64_t k0 = kb + c * 1024 + (int64_t)lane * 16;
            const bool live = k0 < p.K;
            float w[16];
            const u32 ww[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                int code;
                if constexpr (BITS == 8) {
                    const u32 b = (ww[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    code = is_signed ? (int)(int8_t)b : (int)b;
                } else {
                    const u32 b = (ww[j >> 3] >> (4 * (j & 7))) & 15u;
                    code = is_signed ? (int)b - 8 : (int)b;  // packed signed ints are stored as value - min
                }
                w[j] = (float)code;
            }
            if (live) {
                const float sc = scv[c];
                if (zrow) {
                    const float z = zpv[c];
#pragma unroll
                    for (int j = 0; j < 16; ++j) w[j] = fmaf(w[j], sc, z);
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) w[j] = w[j] * sc;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) w[j] = 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = FT<T_ID>::round(w[j]);
            if (log2had) {
                wave_hadamard16(w, log2had, hscale);
#pragma unroll
                for (int j = 0; j < 16; ++j) w[j] = FT<T_ID>::round(w[j]);
            }
            if (!live) continue;
#pragma unroll
            for (int i = 0; i < MROWS; ++i) {
                const int64_t m = (i < M) ? i : M - 1;
                float xv[16];
                if constexpr (PFX) {
                    Vec16<T_ID>::unpack(xr[c][0], xv);
                    Vec16<T_ID>::unpack(xr[c][1], xv + 8);
                } else {
                    load_row16<T_ID>(x, m * ldx + k0, xv);
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[i] = fmaf(xv[j], w[j], acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MROWS; ++i) {
        float sum = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0 && i < M) {
            if (bias) sum += FT<T_ID>::load(bias, n);
            FT<T_ID>::store(out, (int64_t)i * p.N + n, sum);
        }
    }
}

// The few-row linear of HADAMARD layers with the default rotation group 256 (FLUX int4 + Hadamard adaLN projections): the weight row is
// un-rotated on the matrix cores.  linear_skinny_fast_kernel's FWHT (16 elements per lane: two radix-4 stages across lanes = 96 DPP /
// ds_swizzle moves per 16 elements) took 37 of the 59 us of an 18432 x 3072 int4 layer.  Here a wave owns one output channel and
// walks its row group by group in the MFMA layout of hadamard_dev.h: lane l holds the 4 consecutive columns 16 (l & 15) + 4 (l >> 4)
// .. +3 of the group -- 2 bytes of int4 codes / 4 bytes of int8 codes per lane, a whole group = one contiguous 128 / 256 bytes per
// wave-load -- dequantizes them (f32(q) * s | fma, rounded to T: dequantizer.py:27, 63), rotates (five MFMAs, rounded to T:
// dequantizer.py:82-87) and multiplies with the same 4 columns of x.  All loads of up to 16 groups are issued before the first use.
template <int T_ID, int BITS, int MROWS>
__global__ __launch_bounds__(256) void linear_skinny_had256_kernel(const DeqParams p, const void* __restrict__ x, const void* __restrict__ bias,
                                                                   void* __restrict__ out, int64_t M, int64_t ldx) {
    SDNQ_DEQ_ARGS_NOW(p);
    static_assert(T_ID == SDNQ_BF16 || T_ID == SDNQ_F16, "16-bit activations");
    constexpr int NG = 16;
    const int lane = threadIdx.x & 63;
    // the wave's output channel is wave-uniform: pinned to a scalar register, so that the buffer descriptors derived from it live in SGPRs
    // (left as a function of threadIdx.x they were VGPRs, and each of the 48 buffer loads sat in a readfirstlane waterfall loop)
    const int64_t n = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (n >= p.N) return;
    float acc[MROWS];
#pragma unroll
    for (int i = 0; i < MROWS; ++i) acc[i] = 0.0f;
    const int eoff = 16 * (lane & 15) + 4 * (lane >> 4);
    const uint8_t* wrow = (const uint8_t*)p.w + (BITS == 8 ? n * p.K : n * p.K / 2) + (BITS == 8 ? eoff : eoff / 2);
    const float* srow = p.scale + n * p.G;
    const float* zrow = p.zp ? p.zp + n * p.G : nullptr;
    const bool is_signed = p.fmt.kind == SDNQ_KIND_INT;
    // codes -> numbers without branches: int8 two's complement: (byte ^ 0x80) - 128;  uint8: byte;  packed signed nibble: code - 8
    const u32 flip8 = (is_signed && BITS == 8) ? 0x80808080u : 0u;
    const float qsub = is_signed ? (BITS == 8 ? 128.0f : 8.0f) : 0.0f;
    float hf[4];
    had16_operand(lane, hf);
    const int ngroups = (int)(p.K / 256);
    auto rsW = SDNQ_MAKE_RSRC((const uint8_t*)p.w + (BITS == 8 ? n * p.K : n * p.K / 2));
    auto rsS = SDNQ_MAKE_RSRC(srow);
    auto rsZ = SDNQ_MAKE_RSRC(zrow ? zrow : srow);
    auto rsX = SDNQ_MAKE_RSRC(x);
    for (int g0 = 0; g0 < ngroups; g0 += NG) {
        u32 code[NG];
        float sc[NG], zp[NG];
        uint2 xr[NG][MROWS];
#pragma unroll
        for (int g = 0; g < NG; ++g) {  // unconditional, clamped: a group past the end re-reads group 0 and is dropped
            // (buffer loads -- wave-uniform base, 32-bit lane offset, group offset in the scalar operand: a load with a 64-bit VGPR
            //  address waits ~1000 cycles at issue while another wave of the SIMD runs the rotation's MFMAs, sdnq_dev.h)
            const int kk = (g0 + g < ngroups ? g0 + g : 0) * 256;
            if constexpr (BITS == 8) code[g] = (u32)SDNQ_BUF_LOAD4(rsW, eoff, kk);
            else code[g] = (u32)SDNQ_BUF_LOAD2(rsW, eoff / 2, kk / 2);
            const int gi = (kk + eoff) / p.group_size;  // group_size % 4 == 0: the 4 columns share one scale group
            sc[g] = __builtin_bit_cast(float, SDNQ_BUF_LOAD4(rsS, gi * 4, 0));
            zp[g] = zrow ? __builtin_bit_cast(float, SDNQ_BUF_LOAD4(rsZ, gi * 4, 0)) : 0.0f;
#pragma unroll
            for (int i = 0; i < MROWS; ++i) {
                const v2i t = SDNQ_BUF_LOAD8(rsX, (int)((i < M ? i : 0) * ldx + eoff) * 2, kk * 2);
                xr[g][i] = make_uint2((u32)t[0], (u32)t[1]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g0 + g < ngroups) {  // wave-uniform
            // VALU diet (the kernel is VALU + MFMA bound, not HBM bound): codes -> floats with one extract + one convert each, the two
            // roundings to T as PACKED converts whose results feed the MFMA / the dot product directly, x . w as packed dot products
            float w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float q;
                if constexpr (BITS == 8) q = (float)(((code[g] ^ flip8) >> (8 * e)) & 0xffu) - qsub;   // v_cvt_f32_ubyteN
                else q = (float)((code[g] >> (4 * e)) & 15u) - qsub;
                w[e] = zrow ? fmaf(q, sc[g], zp[g]) : q * sc[g];
            }
            const uint2 wp = make_uint2(pack2<T_ID>(w[0], w[1]), pack2<T_ID>(w[2], w[3]));  // the rounding to T (dequantizer.py:27, 63)
            const v4f y = had256_group<T_ID>(wp, hf);
#pragma unroll
            for (int i = 0; i < MROWS; ++i) {
                const u32 y0 = pack2<T_ID>(y[0], y[1]), y1 = pack2<T_ID>(y[2], y[3]);  // the rounding to T after the rotation (:82-87)
                if constexpr (T_ID == SDNQ_BF16) {
                    acc[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, xr[g][i].x), __builtin_bit_cast(v2bf, y0), acc[i], false);
                    acc[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, xr[g][i].y), __builtin_bit_cast(v2bf, y1), acc[i], false);
                } else {
                    acc[i] = __builtin_amdgcn_fdot2(__builtin_bit_cast(v2h, xr[g][i].x), __builtin_bit_cast(v2h, y0), acc[i], false);
                    acc[i] = __builtin_amdgcn_fdot2(__builtin_bit_cast(v2h, xr[g][i].y), __builtin_bit_cast(v2h, y1), acc[i], false);
                }
            }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MROWS; ++i) {
        float sum = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0 && i < M) {
            if (bias) sum += FT<T_ID>::load(bias, n);
            FT<T_ID>::store(out, (int64_t)i * p.N + n, sum);
        }
    }
}

// Few-row linear on an int8 row-wise weight WITH SVD factors (the M < 32 branch of an SVD layer, e.g. FLUX adaLN projections):
// y = x . W^T + b with W = round(round(q * s) + svd_up . svd_down) exactly as sdnq_hip_dequant forms it (dequantizer.py:79-83),
// but the rank-R product is done on the matrix cores tile by tile and W never exists in memory.  One workgroup = 32 output
// channels; its 4 waves split K in blocks of 32.  Per block: D[k][n] = down_t[k][:] . up[n][:] (R/16 MFMAs, operands are
// 16-byte rows of down_t [K][R] and svd_up [N][R]); lane (n = lane & 31, half = lane >> 5) then owns k = (reg & 3) + 8 (reg >> 2)
// + 4 half of that tile, decodes the matching 4 x 4 int8 codes of row n, forms W and multiplies by x (f32 copy in LDS).
// HBM-bound on the codes: N*K bytes (the dequantize + GEMV pair it replaces moves 5 N*K bytes and is VALU-bound on the rank loop).
template <bool IS_BF16, int MR, int BITS>
__global__ __launch_bounds__(256) void skinny_svd_kernel(const DeqParams p, const uint16_t* __restrict__ down_t, const void* __restrict__ x,
                                                         const void* __restrict__ bias, void* __restrict__ out, int64_t M, int64_t ldx) {
    constexpr int T_ID = IS_BF16 ? SDNQ_BF16 : SDNQ_F16;
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [MR][K]
    __shared__ float red[4][MR][32];
    const int tid = threadIdx.x, lane = tid & 63, nl = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = (int)p.K, R = p.rank;
    for (int i = tid; i < MR * K; i += 256) {
        const int m = i / K, k = i - m * K;
        xs[i] = (m < M) ? FT<T_ID>::load(x, (int64_t)m * ldx + k) : 0.0f;
    }
    __syncthreads();
    int64_t gn = (int64_t)blockIdx.x * 32 + nl;
    const bool n_ok = gn < p.N;
    if (!n_ok) gn = p.N - 1;
    const float* srow = p.scale + gn * p.G;
    const float* zrow = p.zp ? p.zp + gn * p.G : nullptr;
    const bool is_signed = p.fmt.kind == SDNQ_KIND_INT;
    const uint16_t* up = (const uint16_t*)p.svd_up + gn * R + hi * 8;
    const uint8_t* wrow = (const uint8_t*)p.w + (BITS == 8 ? gn * K : gn * K / 2);
    float acc[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
    for (int k0 = wave * 32; k0 < K; k0 += 128) {
        v16f ud;
#pragma unroll
        for (int e = 0; e < 16; ++e) ud[e] = 0.0f;
        const uint16_t* dn = down_t + (int64_t)(k0 + nl) * R + hi * 8;
        for (int kr = 0; kr < R; kr += 16) {
            const uint4 fd = *(const uint4*)(dn + kr), fu = *(const uint4*)(up + kr);
            if constexpr (IS_BF16) ud = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, fd), __builtin_bit_cast(v8bf, fu), ud, 0, 0, 0);
            else ud = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, fd), __builtin_bit_cast(v8h, fu), ud, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int kb = k0 + 8 * g + 4 * hi;  // 4 consecutive columns: one scale group (group_size % 4 == 0)
            const float s = srow[kb / p.group_size];
            const float z = zrow ? zrow[kb / p.group_size] : 0.0f;
            u32 w4;
            if constexpr (BITS == 8) w4 = *(const u32*)(wrow + kb);
            else w4 = *(const uint16_t*)(wrow + kb / 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float q;
                if constexpr (BITS == 8) q = is_signed ? (float)(int)(int8_t)(w4 >> (8 * e)) : (float)((w4 >> (8 * e)) & 0xffu);
                else q = is_signed ? (float)((int)((w4 >> (4 * e)) & 15u) - 8) : (float)((w4 >> (4 * e)) & 15u);  // packed signed: value - min
                float wv = FT<T_ID>::round(zrow ? fmaf(q, s, z) : q * s);  // dequantize -> .to(svd dtype)
                wv = FT<T_ID>::round(wv + ud[4 * g + e]);                // addmm_(svd_up, svd_down): one rounding of the sum
#pragma unroll
                for (int m = 0; m < MR; ++m) acc[m] = fmaf(xs[m * K + kb + e], wv, acc[m]);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        acc[m] += __shfl_xor(acc[m], 32, 64);
        if (hi == 0) red[wave][m][nl] = acc[m];
    }
    __syncthreads();
    if (tid < 32 * MR) {
        const int m = tid / 32, n = tid % 32;
        const int64_t on = (int64_t)blockIdx.x * 32 + n;
        if (m < M && on < p.N) {
            float sum = (red[0][m][n] + red[1][m][n]) + (red[2][m][n] + red[3][m][n]);
            if (bias) sum += FT<T_ID>::load(bias, on);
            FT<T_ID>::store(out, (int64_t)m * p.N + on, sum);
        }
    }
}

// The same few-row SVD linear for the default rank R = 32, fed by LDS-DMA.  skinny_svd_kernel above loads 4 bytes per lane per load
// and waits for every 32-k block's loads before using them: 24 dependent memory round trips per wave, 76 us for FLUX's 18432 x 3072
// modulation layers against 14 us of weight traffic.  Here every wave owns a private ring of D stages (one 32-k block each: the
// block's codes, 32 rows x 32 bytes, and its 32 rows of down_t, 64 bytes each = 3 LDS-DMAs of 1 KB), D - 1 blocks in flight, no
// workgroup barrier in the loop (a wave only reads what it fetched itself).  The MFMA's k rows are fed in a PERMUTED order --
// A-operand row i carries k = 16 ((i >> 2) & 1) + 4 (i >> 3) + (i & 3) -- so that the 16 accumulator registers of lane (n = lane &
// 31, half = lane >> 5) are the 16 CONSECUTIVE columns 16 half .. 16 half + 15 of row n: one 16-byte LDS read fetches their codes.
// LDS swizzles (applied on the global side of the DMA, LDS stays lane-linear): codes: 16-byte half ^= (row >> 3) & 1; down_t:
// 16-byte chunk ^= (row >> 2) & 3.
template <bool IS_BF16, int MR, int BITS>
__global__ __launch_bounds__(256) void skinny_svd32_kernel(const DeqParams p, const uint16_t* __restrict__ down_t, const void* __restrict__ x,
                                                           const void* __restrict__ bias, void* __restrict__ out, int64_t M, int64_t ldx) {
    SDNQ_DEQ_ARGS_NOW(p);
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int T_ID = IS_BF16 ? SDNQ_BF16 : SDNQ_F16;
    constexpr int D = 4, STG = 3072, R = 32;
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];  // [4 waves][D][STG] rings, xs [MR][K] f32, scales / zero points [32][G] f32 each
    __shared__ float red[4][MR][32];
    const int tid = threadIdx.x, lane = tid & 63, nl = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = (int)p.K;
    uint8_t* ring = smem + wave * (D * STG);
    uint16_t* xs = (uint16_t*)(smem + 4 * D * STG);  // [MR][K] activations, 16-bit
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    // ---- DMA roles
    const uint8_t* wsrc;  // this lane's code bytes of block 0
    if constexpr (BITS == 8) {
        const int r = lane >> 1, lh = (lane & 1) ^ ((r >> 3) & 1);
        int64_t g = n0 + r;
        if (g >= p.N) g = p.N - 1;
        wsrc = (const uint8_t*)p.w + g * K + 16 * lh;
    } else {  // 32 rows x 16 bytes = half a DMA: the upper 32 lanes fetch the same bytes again (their LDS kilobyte half is not read)
        int64_t g = n0 + (lane & 31);
        if (g >= p.N) g = p.N - 1;
        wsrc = (const uint8_t*)p.w + g * (K / 2);
    }
    const int drow = lane >> 2, dchunk = lane & 3;  // down_t piece a: row 16 a + drow, physical chunk dchunk
    const uint16_t* dsrc0 = down_t + (int64_t)drow * R + ((dchunk ^ ((drow >> 2) & 3)) << 3);
    const uint16_t* dsrc1 = down_t + (int64_t)(16 + drow) * R + ((dchunk ^ (((16 + drow) >> 2) & 3)) << 3);
    const int nblk = K / 32, nit = (nblk + 3) / 4;
    auto issue = [&](int it) {  // block 4 it + wave; past the end of K: the last block again (dropped by `live` below)
        int b = 4 * it + wave;
        if (b >= nblk) b = nblk - 1;
        uint8_t* base = ring + (it % D) * STG;
        const int k0 = b * 32;
        __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + (BITS == 8 ? k0 : k0 / 2)), (lptr_t)base, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(dsrc0 + (int64_t)k0 * R), (lptr_t)(base + 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(dsrc1 + (int64_t)k0 * R), (lptr_t)(base + 2048), 16, 0, 0);
    };
#pragma unroll
    for (int s0 = 0; s0 < D - 1; ++s0) issue(s0);
    // ---- x in LDS as it is (16-bit elements; rows past M are zero) while the first blocks are in flight: 16-byte pieces, four loads
    // per thread in flight (an element-at-a-time loop waits one memory round trip per element: 12 of them for K = 3072)
    {
        const int kc = K / 8, total = MR * kc;  // 16-byte pieces
        for (int c0 = tid; c0 < total; c0 += 4 * 256) {
            uint4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 256 < total ? c0 + j * 256 : 0;
                const int m = c / kc, k8 = c - m * kc;
                v[j] = *(const uint4*)((const uint16_t*)x + (int64_t)(m < M ? m : 0) * ldx + k8 * 8);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 256;
                if (c < total) *(uint4*)(xs + c * 8) = (c / kc < M) ? v[j] : make_uint4(0, 0, 0, 0);
            }
        }
    }
    // scales / zero points of the 32 rows in LDS: a global load inside the K loop would make the compiler drain the DMA ring
    // (s_waitcnt vmcnt(0)) at its first use
    const int G = p.G;
    float* s_sc = (float*)(xs + MR * K);
    float* s_zp = s_sc + 32 * G;
    for (int i = tid; i < 32 * G; i += 256) {
        int64_t g = n0 + i / G;
        if (g >= p.N) g = p.N - 1;
        s_sc[i] = p.scale[g * G + i % G];
        s_zp[i] = p.zp ? p.zp[g * G + i % G] : 0.0f;  // fma(q, s, +0) == q * s
    }
    int64_t gn = n0 + nl;
    if (gn >= p.N) gn = p.N - 1;
    // codes -> numbers without branches: int8 two's complement: (byte ^ 0x80) - 128;  uint8: byte;  packed signed nibble: code - 8
    const bool is_signed = p.fmt.kind == SDNQ_KIND_INT;
    const u32 flip = (is_signed && BITS == 8) ? 0x80808080u : 0u;
    const float qsub = is_signed ? (BITS == 8 ? 128.0f : 8.0f) : 0.0f;
    const float inv_group = 1.0f / (float)p.group_size;
    const uint16_t* up = (const uint16_t*)p.svd_up + gn * R + hi * 8;
    const v4i fu0 = *(const v4i*)up, fu1 = *(const v4i*)(up + 16);
    // fragment reads: A row of this lane = the permuted k row; code bytes of row nl
    const int krow = 16 * ((nl >> 2) & 1) + 4 * (nl >> 3) + (nl & 3);
    const int a_off0 = 1024 + krow * 64 + (((0 + hi) ^ ((krow >> 2) & 3)) << 4);
    const int a_off1 = 1024 + krow * 64 + (((2 + hi) ^ ((krow >> 2) & 3)) << 4);
    const int w_off = BITS == 8 ? nl * 32 + ((hi ^ ((nl >> 3) & 1)) << 4) : nl * 16 + hi * 8;
    float acc[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
    __syncthreads();  // xs complete
    for (int it = 0; it < nit; ++it) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 2) * 3) : "memory");  // this wave's block `it` has landed
        issue(it + D - 1);  // refills the slot read in the previous iteration (its reads fed arithmetic already)
        const uint8_t* base = ring + (it % D) * STG;
        if (4 * it + wave >= nblk) continue;  // wave-uniform: a block past the end of K (its DMAs re-fetched the last block)
        const int kb = (4 * it + wave) * 32 + 16 * hi;  // this lane's 16 consecutive columns: one scale group (group_size % 16 == 0)
        v16f ud;
#pragma unroll
        for (int e = 0; e < 16; ++e) ud[e] = 0.0f;
        const v4i fd0 = *(const v4i*)(base + a_off0), fd1 = *(const v4i*)(base + a_off1);
        if constexpr (IS_BF16) {
            ud = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, fd0), __builtin_bit_cast(v8bf, fu0), ud, 0, 0, 0);
            ud = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, fd1), __builtin_bit_cast(v8bf, fu1), ud, 0, 0, 0);
        } else {
            ud = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, fd0), __builtin_bit_cast(v8h, fu0), ud, 0, 0, 0);
            ud = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, fd1), __builtin_bit_cast(v8h, fu1), ud, 0, 0, 0);
        }
        u32 ww[4];
        if constexpr (BITS == 8) { const v4i t4 = *(const v4i*)(base + w_off); ww[0] = t4[0]; ww[1] = t4[1]; ww[2] = t4[2]; ww[3] = t4[3]; }
        else { const v2i t2 = *(const v2i*)(base + w_off); ww[0] = t2[0]; ww[1] = t2[1]; ww[2] = 0; ww[3] = 0; }
        const int gi = (int)(((float)kb + 0.5f) * inv_group);  // kb / group_size (exact: both are multiples of 16, K < 2^20)
        const float sc = s_sc[nl * G + gi], zc = s_zp[nl * G + gi];
        // VALU diet (the kernel is bound by the per-element arithmetic, ~14 instructions before): codes -> floats with one
        // v_cvt_f32_ubyteN each, both roundings to T as PACKED converts of a column pair, the products as packed dot products
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32 xq[MR][2];  // columns (4 g, 4 g + 1) and (4 g + 2, 4 g + 3) of every activation row, as stored
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                const v2i t2 = *(const v2i*)(xs + m * K + kb + 4 * g);
                xq[m][0] = (u32)t2[0];
                xq[m][1] = (u32)t2[1];
            }
            u32 cw;  // the 4 codes of columns 4 g .. 4 g + 3, one per byte
            if constexpr (BITS == 8) {
                cw = ww[g] ^ flip;
            } else {
                const u32 n4 = (ww[g >> 1] >> (16 * (g & 1))) & 0xffffu;  // 4 nibbles -> 4 bytes
                cw = (n4 & 0xfu) | ((n4 & 0xf0u) << 4) | ((n4 & 0xf00u) << 8) | ((n4 & 0xf000u) << 12);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float q0 = (float)((cw >> (16 * h)) & 0xffu) - qsub, q1 = (float)((cw >> (16 * h + 8)) & 0xffu) - qsub;
                float b0 = fmaf(q0, sc, zc), b1 = fmaf(q1, sc, zc);
                if constexpr (!IS_BF16) {
                    // float16: the reference rounds the fma to float32 and THAT to float16 (addcmul in float32, then .to(), dequantizer.py:27).
                    // Left visible to the compiler, fma + conversion fold into one v_fma_mixlo_f16, which rounds the exact q s + z ONCE:
                    // another float16 whenever the float32 rounding lands on a float16 tie (profiles/skinny_census.md)
                    asm("" : "+v"(b0));
                    asm("" : "+v"(b1));
                }
                const u32 pw = pack2<T_ID>(b0, b1);  // dequantize -> .to(svd dtype)
                float r0, r1;
                if constexpr (IS_BF16) { r0 = __uint_as_float(pw << 16); r1 = __uint_as_float(pw & 0xffff0000u); }
                else { r0 = f16_bits_to_f32((uint16_t)pw); r1 = f16_bits_to_f32((uint16_t)(pw >> 16)); }
                const u32 ps = pack2<T_ID>(r0 + ud[4 * g + 2 * h], r1 + ud[4 * g + 2 * h + 1]);  // addmm_: one rounding of the sum
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    if constexpr (IS_BF16) acc[m] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, xq[m][h]), __builtin_bit_cast(v2bf, ps), acc[m], false);
                    else acc[m] = __builtin_amdgcn_fdot2(__builtin_bit_cast(v2h, xq[m][h]), __builtin_bit_cast(v2h, ps), acc[m], false);
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing refills
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        acc[m] += __shfl_xor(acc[m], 32, 64);
        if (hi == 0) red[wave][m][nl] = acc[m];
    }
    __syncthreads();
    if (tid < 32 * MR) {
        const int m = tid / 32, n = tid % 32;
        const int64_t on = n0 + n;
        if (m < M && on < p.N) {
            float sum = (red[0][m][n] + red[1][m][n]) + (red[2][m][n] + red[3][m][n]);
            if (bias) sum += FT<T_ID>::load(bias, on);
            FT<T_ID>::store(out, (int64_t)m * p.N + on, sum);
        }
    }
}

}  // namespace

extern "C" int sdnq_hip_linear_skinny_svd(const SdnqWeight* w, const void* svd_down_t, const void* x, const void* bias, int dtype,
                                          void* out, int64_t m, int64_t ldx, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!x || !out || !svd_down_t || !w->svd_up) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (w->svd_dtype != dtype) return SDNQ_ERR_DTYPE;
    if (p.sdt != SDNQ_F32 && p.sdt != dtype) return SDNQ_ERR_DTYPE;  // 16-bit scales: q * s is rounded to the scale dtype = svd dtype here
    const int bits = int_code_bits(p);
    if (!bits || (p.group_size % 4) != 0 || p.P != 1) return SDNQ_ERR_UNSUPPORTED;
    if (m <= 0 || m > 4 || ldx < p.K || (p.K % 32) != 0 || p.rank <= 0 || (p.rank % 16) != 0) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)svd_down_t % 16) || ((uintptr_t)w->svd_up % 16)) return SDNQ_ERR_ALIGN;
    const int rows = m <= 1 ? 1 : (m <= 2 ? 2 : 4);  // MR of both kernels: one workgroup column covers every row
    const size_t lds = (size_t)rows * p.K * sizeof(float);
    if (lds > 150 * 1024) return SDNQ_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((p.N + 31) / 32)), block(256);
    // skinny_svd32_kernel: x as 16-bit elements + the four private DMA rings + the rows' scales / zero points
    const size_t lds32 = lds / 2 + 4 * 4 * 3072 + (size_t)32 * p.G * 8;
    const bool rank32 = p.rank == 32 && lds32 <= 150 * 1024 && (p.group_size % 16) == 0 && p.G <= 64 && (p.K % 32) == 0 &&
                        (bits == 8 || (p.K % 64) == 0) && ((uintptr_t)x % 16) == 0 && ((ldx * 2) % 16) == 0;
    const size_t dyn = rank32 ? lds32 : lds;
    const bool launched = dispatch_int<SDNQ_BF16, SDNQ_F16>(dtype, [&](auto T) {
        return dispatch_int<1, 2, 4>(rows, [&](auto MR) {
            return dispatch_int<8, 4>(bits, [&](auto B) {
                constexpr bool bf16 = T.value == SDNQ_BF16;
                auto kern = rank32 ? skinny_svd32_kernel<bf16, MR.value, B.value> : skinny_svd_kernel<bf16, MR.value, B.value>;
                if (dyn > 64 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess)
                    return false;
                hipLaunchKernelGGL(kern, grid, block, dyn, s, p, (const uint16_t*)svd_down_t, x, bias, out, m, ldx);
                return true;
            });
        });
    });
    if (!launched) return SDNQ_ERR_LAUNCH;
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_linear_skinny(const SdnqWeight* w, int hadamard_group, const void* x, const void* bias, int dtype, void* out,
                                      int64_t m, int64_t ldx, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!x || !out) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    if (m <= 0 || m > 64 || ldx < p.K) return SDNQ_ERR_SHAPE;
    if (w->svd_up) return SDNQ_ERR_UNSUPPORTED;  // the SVD term needs the dequantize-then-GEMM path
    const int log2had = hadamard_log2(hadamard_group, p.K);
    if (log2had < 0) return SDNQ_ERR_SHAPE;
    const int eb = (dtype == SDNQ_F32) ? 4 : 2;
    if (((uintptr_t)x % 16) || ((ldx * eb) % 16)) return SDNQ_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((p.N + 3) / 4)), block(256);
    const int bits = int_code_bits(p);
    static const int had_mfma = [] { const char* e = getenv("SDNQ_HIP_HADAMARD_MFMA"); return e ? atoi(e) : 1; }();
    // The two tuned kernels: int8 / int4 codes, at most 4 rows, all of them in one launch column (MROWS 1 / 2 / else 4).  (They round
    // q * s straight to the activation dtype: with 16-bit scales that is the scale dtype's rounding too.)
    const bool tuned = bits && m <= 4 && p.P == 1 && (p.sdt == SDNQ_F32 || p.sdt == dtype);
    const int rows_tuned = m == 1 ? 1 : (m == 2 ? 2 : 4);
    if (tuned && hadamard_group == 256 && dtype != SDNQ_F32 && (p.group_size % 4) == 0 && had_mfma && ((uintptr_t)x % 8) == 0 &&
        ((ldx * 2) % 8) == 0) {
        dispatch_int<SDNQ_BF16, SDNQ_F16>(dtype, [&](auto T) {
            return dispatch_int<8, 4>(bits, [&](auto B) {
                return dispatch_int<1, 2, 4>(rows_tuned, [&](auto MR) {
                    hipLaunchKernelGGL((linear_skinny_had256_kernel<T.value, B.value, MR.value>), grid, block, 0, s, p, x, bias, out, m, ldx);
                    return true;
                });
            });
        });
    } else if (tuned && (p.group_size % 16) == 0 && (p.K % 16) == 0) {
        dispatch_float(dtype, [&](auto T) {
            return dispatch_int<8, 4>(bits, [&](auto B) {
                return dispatch_int<1, 2, 4>(rows_tuned, [&](auto MR) {
                    hipLaunchKernelGGL((linear_skinny_fast_kernel<T.value, B.value, MR.value>), grid, block, 0, s, p, x, bias, out, m, ldx, log2had);
                    return true;
                });
            });
        });
    } else {
        const int rows = m == 1 ? 1 : (m <= 2 ? 2 : (m <= 4 ? 4 : 8));  // the generic kernel: grid.y walks M in chunks of MROWS
        grid.y = (unsigned)((m + rows - 1) / rows);
        dispatch_float(dtype, [&](auto T) {
            return dispatch_int<1, 2, 4, 8>(rows, [&](auto MR) {
                hipLaunchKernelGGL((linear_skinny_kernel<T.value, MR.value>), grid, block, 0, s, p, x, bias, out, m, ldx, log2had);
                return true;
            });
        });
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
