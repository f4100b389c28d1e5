// Dequantize family for gfx950: kernels that stream a stored weight once and write (or score) its values.
//
//   sdnq_hip_dequant   <- SDNQDequantizer.__call__ / dequantize_weight   (dequantizer.py:135-162, 389-429)
//                         dequantize_symmetric :52-84, dequantize_asymmetric :15-48
//   sdnq_hip_embedding <- quantized_embedding (layers/embedding/forward.py:14-68): weight[ids] dequantized, one launch
//   sdnq_hip_dequant_loss <- mse_loss(W, dequantize(q)) of the dynamic dtype search (quantizer.py:384-400), fused, deterministic
//   sdnq_hip_requant   <- re_quantize_matmul -> re_quantize_int_mm / re_quantize_fp_mm
//                         (dequantizer.py:204-239, 166-174, 190-201; quantize_int_mm quant_utils.py:265-273)
//   sdnq_hip_lut4_build <- the same re-quantization kept as 16-entry tables for the GEMM that expands 4-bit codes itself (gemm_w4.hip)
//   sdnq_hip_unpack_mm <- the stored codes as a matmul operand, no scaling (linear_int8.py:46, linear_fp16.py:27-31)
//
// All are HBM-streaming kernels on dequant16 (weight_dev.h): a thread owns 16 consecutive elements of one weight row (a whole number
// of codec groups for every packed format), so packed reads are contiguous per lane and outputs are 16/32/64-byte lane-contiguous
// vectors.  The few-row linears on stored codes are in skinny.hip, the float linears in linear_float.hip.
#include "hadamard_dev.h"
#include "weight_dev.h"

namespace {

template <int OUT_T, int SVD_T>
__global__ __launch_bounds__(256) void dequant_kernel(const DeqParams p, void* __restrict__ out) {
    const int64_t units_per_row = p.K / 16;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= p.N * units_per_row) return;
    int64_t n, k0;
    divmod(u, units_per_row, n, k0);  // (32-bit whenever it fits, sdnq_dev.h)
    k0 *= 16;
    float v[16];
    dequant16(p, n, k0, v);
    if (p.svd_up) {
        // result.to(svd dtype).addmm_(svd_up, svd_down): one rounding of W, fp32 accumulate, one rounding of the sum
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) { v[j] = FT<SVD_T>::round(v[j]); acc[j] = 0.0f; }
        for (int r = 0; r < p.rank; ++r) {
            const float up = FT<SVD_T>::load(p.svd_up, n * p.rank + r);
            float dn[16];  // svd_down[r][k0 .. k0+15] (k0 % 16 == 0, K % 16 == 0)
            load_row16<SVD_T>(p.svd_down, (int64_t)r * p.K + k0, dn);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = fmaf(up, dn[j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = FT<SVD_T>::round(v[j] + acc[j]);
    }
    uint8_t* o = (uint8_t*)out + (n * p.K + k0) * FT<OUT_T>::bytes;
    if constexpr (OUT_T == SDNQ_F32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *(uint4*)(o + 16 * q) = Vec16<SDNQ_F32>::pack(v + 4 * q);
    } else {
        *(uint4*)o = Vec16<OUT_T>::pack(v);
        *(uint4*)(o + 16) = Vec16<OUT_T>::pack(v + 8);
    }
}

// Gather-dequantize of an embedding table (layers/embedding/forward.py:14-68): one wave per (id, 1024-column chunk of the row),
// a lane owns 16 consecutive columns.  Only the gathered rows of codes / scales / zero points / svd_up are read; svd_down [R][D]
// is shared by every row and stays in L2.  The read row is clamped to [0, V-1], so no address leaves the table; an id outside
// [0, V) writes a row of NaN instead.  Rounding order of the reference on weight[ids] (dequantizer.py:15-84):
//   v = w * s (+ zp) in the scale dtype (dequant16)
//   SVD, table not grouped:  v = round_svd(round_svd(v) + sum_r up[r] * down[r])          result.to(svd dtype).addmm_(up, down)
//   SVD, grouped table:      v = round_sdt(v + round_svd(sum_r up[r] * down[r]))           the 3-D weight[ids] takes the
//                            `is_conv` branch: result.add_(torch.mm(up, down).unflatten(..)) in the scale dtype
//   cast to OUT_T; Hadamard rotation in OUT_T (wave_hadamard16: the arithmetic of sdnq_hip_hadamard); v = round(v * embed_scale)
template <int OUT_T, int SVD_T>
__global__ __launch_bounds__(256) void embedding_kernel(const DeqParams p, const void* __restrict__ ids, int ids64, int64_t n_ids,
                                                        int log2g, int has_es, float es, void* __restrict__ out) {
    const int64_t chunks = (p.K + 1023) / 1024;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= n_ids * chunks) return;  // wave-uniform: the lanes that stay run the cross-lane rotation together
    int64_t i, c;
    divmod(wave, chunks, i, c);
    const int64_t id = ids64 ? ((const int64_t*)ids)[i] : (int64_t)((const int32_t*)ids)[i];
    const bool valid = id >= 0 && id < p.N;
    const int64_t row = id < 0 ? 0 : (id >= p.N ? p.N - 1 : id);
    const int64_t k0 = c * 1024 + (threadIdx.x & 63) * 16;
    const bool active = k0 < p.K;
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = 0.0f;
    if (active) {
        dequant16(p, row, k0, v);
        if (p.svd_up) {
            float acc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
            for (int r = 0; r < p.rank; ++r) {
                const float up = FT<SVD_T>::load(p.svd_up, row * p.rank + r);
                float dn[16];  // svd_down[r][k0 .. k0+15] (k0 % 16 == 0, K % 16 == 0)
                load_row16<SVD_T>(p.svd_down, (int64_t)r * p.K + k0, dn);
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[j] = fmaf(up, dn[j], acc[j]);
            }
            if (p.G > 1) {
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = round_rt(v[j] + FT<SVD_T>::round(acc[j]), p.sdt);
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = FT<SVD_T>::round(FT<SVD_T>::round(v[j]) + acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = FT<OUT_T>::round(v[j]);
    if (log2g) {
        wave_hadamard16(v, log2g, hadamard_scale(log2g, OUT_T));
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = FT<OUT_T>::round(v[j]);
    }
    if (has_es) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = FT<OUT_T>::round(v[j] * es);
    }
    if (!valid) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = __builtin_nanf("");
    }
    if (!active) return;
    uint8_t* o = (uint8_t*)out + (i * p.K + k0) * FT<OUT_T>::bytes;
    if constexpr (OUT_T == SDNQ_F32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *(uint4*)(o + 16 * q) = Vec16<SDNQ_F32>::pack(v + 4 * q);
    } else {
        *(uint4*)o = Vec16<OUT_T>::pack(v);
        *(uint4*)(o + 16) = Vec16<OUT_T>::pack(v + 8);
    }
}

// Reconstruction loss of a quantized weight (sdnq_hip_dequant_loss): sum over [N][K] of (deq - ref)^2 without writing deq.  One wave
// per (row, 1024-column chunk) as in embedding_kernel, a grid-stride loop over the chunks; a lane owns 16 consecutive columns, so a
// Hadamard group (<= 512 columns, dividing K) lies inside one wave's chunk and is undone in registers.  deq is formed exactly as
// dequant_kernel<SDNQ_F32, SVD_T> forms it (2-D SVD rounding: round_svd(round_svd(v) + sum_r up * down)), then rotated by
// wave_hadamard16 in fp32 -- the butterflies of hadamard_kernel<SDNQ_F32> (sdnq_hip_hadamard) in the same order.  Each term is
// (d * d) in fp32, as mse_loss computes it, accumulated in fp64 per lane; the 256 lanes are added by a fixed tree and each
// workgroup writes one partial: no atomics, the same bits on every call.
constexpr int kLossMaxBlocks = 2048;  // 8 workgroups of 4 waves per CU on 256 CUs: enough loads in flight to stream HBM

__host__ __device__ inline int64_t loss_blocks(int64_t n, int64_t k) {
    const int64_t waves = n * ((k + 1023) / 1024);
    const int64_t b = (waves + 3) / 4;
    return b < kLossMaxBlocks ? b : kLossMaxBlocks;
}

template <int REF_T, int SVD_T>
__global__ __launch_bounds__(256) void dequant_loss_kernel(const DeqParams p, const void* __restrict__ ref, int64_t ld_ref, int log2g,
                                                           double* __restrict__ partial) {
    __shared__ double red[256];
    const int lane = threadIdx.x & 63;
    const int64_t chunks = (p.K + 1023) / 1024;
    const int64_t total = p.N * chunks;
    const int64_t stride = (int64_t)gridDim.x * 4;
    double acc = 0.0;
    for (int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wave < total; wave += stride) {  // wave-uniform trip count
        int64_t n, c;
        divmod(wave, chunks, n, c);
        const int64_t k0 = c * 1024 + lane * 16;
        const bool active = k0 < p.K;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = 0.0f;
        if (active) {
            dequant16(p, n, k0, v);
            if (p.svd_up) {
                float sacc[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) { v[j] = FT<SVD_T>::round(v[j]); sacc[j] = 0.0f; }
                for (int r = 0; r < p.rank; ++r) {
                    const float up = FT<SVD_T>::load(p.svd_up, n * p.rank + r);
                    float dn[16];  // svd_down[r][k0 .. k0+15] (k0 % 16 == 0, K % 16 == 0)
                    load_row16<SVD_T>(p.svd_down, (int64_t)r * p.K + k0, dn);
#pragma unroll
                    for (int j = 0; j < 16; ++j) sacc[j] = fmaf(up, dn[j], sacc[j]);
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = FT<SVD_T>::round(v[j] + sacc[j]);
            }
        }
        // inactive lanes (the tail chunk of a row) hold zeros and join the cross-lane butterflies; their groups are all inactive
        if (log2g) wave_hadamard16(v, log2g, hadamard_scale(log2g, SDNQ_F32));
        if (active) {
            float rv[16];
            load_row16<REF_T>(ref, n * ld_ref + k0, rv);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float d = v[j] - rv[j];
                acc += (double)(d * d);
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// the partials of dequant_loss_kernel in a fixed order: lane t adds t, t + 256, ... in turn, then the same tree
__global__ __launch_bounds__(256) void loss_sum_kernel(const double* __restrict__ partial, int64_t nparts, double* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// one wave per weight row: phase 1 amax of the fp32 dequant, phase 2 quantize (recompute, L2-hot)
// ASYM = re_quantize_uint_mm (dequantizer.py:178-187): int8 codes of (w - zero_point) / scale with the row's min / max range
template <int MM, bool ASYM = false>
__global__ __launch_bounds__(256) void requant_kernel(const DeqParams p, uint8_t* __restrict__ wq, float* __restrict__ ws,
                                                      float* __restrict__ wzp) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= p.N) return;
    const int64_t npass = (p.K + 1023) / 1024;
    float amax = 0.0f, vmin = 3.4e38f, vmax = -3.4e38f;
    for (int64_t ps = 0; ps < npass; ++ps) {
        const int64_t k0 = ps * 1024 + lane * 16;
        if (k0 < p.K) {
            float v[16];
            dequant16(p, n, k0, v);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if constexpr (ASYM) { vmin = fminf(vmin, v[j]); vmax = fmaxf(vmax, v[j]); }
                else amax = fmaxf(amax, fabsf(v[j]));
            }
        }
    }
    float scale, zpv = 0.0f;
    if constexpr (ASYM) {
        vmin = wave_min(vmin);
        vmax = wave_max(vmax);
        // get_scale_asymmetric (quant_utils.py:10-19) with the int8 range; zero_point.sub_(scale, alpha=-128): 128 * scale is exact.
        // A 16-bit scale dtype (dequantize_fp32=False) rounds sub_, div_ and the alpha-sub once each (round_rt is the identity for f32)
        scale = round_rt(round_rt(vmax - vmin, p.sdt) / 255.0f, p.sdt);
        zpv = round_rt(fmaf(128.0f, scale, vmin), p.sdt);
        if (lane == 0) wzp[n] = zpv;
    } else {
        amax = wave_max(amax);
        const float qmax = (MM == SDNQ_MM_I8) ? 127.0f : 448.0f;
        scale = round_rt(amax / qmax, p.sdt);  // 16-bit scale_dtype: quantize_int_mm / quantize_fp_mm run in that dtype
    }
    if (lane == 0) ws[n] = scale;
    for (int64_t ps = 0; ps < npass; ++ps) {
        const int64_t k0 = ps * 1024 + lane * 16;
        if (k0 < p.K) {
            float v[16];
            dequant16(p, n, k0, v);
            u32 o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                u32 byte;
                if constexpr (MM == SDNQ_MM_I8) {
                    float q = __builtin_rintf(round_rt((ASYM ? round_rt(v[j] - zpv, p.sdt) : v[j]) / scale, p.sdt));
                    if (q != q) q = 0.0f;  // 0/0 of a constant row: NaN.to(int8) is 0 in the reference
                    q = fminf(fmaxf(q, -128.0f), 127.0f);
                    byte = (u32)(int)q & 0xffu;
                } else {
                    float q = round_rt(v[j] / scale, p.sdt);
                    if (q != q) q = 0.0f;
                    q = fminf(fmaxf(q, -448.0f), 448.0f);
                    byte = f32_to_e4m3fn_clamped(q);
                }
                o[j >> 2] |= byte << (8 * (j & 3));
            }
            *(uint4*)(wq + n * p.K + k0) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// Re-quantization of 4-BIT weights through a 16-entry table per (row, group) (round 3; verdict item "LUT re-quantization").
// A 4-bit code has 16 values, so within one quantization group of one row the re-quantized int8 / fp8 byte takes at most 16
// distinct values: instead of one exact division per ELEMENT (64 per group of 64), the four lanes that hold a group compute four
// table entries each -- with the very expression of requant_kernel, so the bytes are identical by construction -- swap them with
// three DPP quad moves, and expand their 16 codes through v_perm byte look-ups.  `ws_known`: the row scales were computed before
// (they depend only on the static weights) and are read from `ws` instead of being derived in a first pass over the row: the
// per-call path of SDNQ_HIP_CACHE_WEIGHTS=0 then reads the codes once.  Needs packed 4-bit storage, group_size % 64 == 0, P == 1.
template <int MM, int NP>
__global__ __launch_bounds__(256) void requant_lut4_kernel(const DeqParams p, uint8_t* __restrict__ wq, float* __restrict__ ws, int ws_known, u32* __restrict__ lut) {
    SDNQ_DEQ_ARGS_NOW(p);
    SDNQ_KERNARGS_NOW("s"(wq), "s"(ws), "s"(ws_known), "s"(lut));
    // NP = passes of 1024 elements per row (K <= 1024 NP), compile time: every load of the row -- codes and group scales of all
    // passes -- is issued before the first use (unconditionally, from clamped addresses: a load under a condition gets its own
    // vmcnt(0)), so a row costs one memory round trip instead of one per pass
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= p.N) return;
    const float* srow = p.scale + n * p.SG;
    const float* zrow = p.zp ? p.zp + n * p.SG : nullptr;
    const uint8_t* crow = (const uint8_t*)p.w + ((n * p.K) >> 1);
    uint2 cw[NP];
    float sg[NP], zg[NP];
    int gb[NP];  // codebooks: offset of the group's 16 levels in the row's table
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        int64_t k0 = (int64_t)ps * 1024 + lane * 16;
        if (k0 >= p.K) k0 = p.K - 16;  // out-of-range lanes read the row's last run and store nothing
        const int g = (int)(k0 / p.group_size);
        cw[ps] = *(const uint2*)(crow + (k0 >> 1));
        gb[ps] = g * 16;
        sg[ps] = p.L ? 0.0f : srow[g];
        zg[ps] = zrow ? zrow[g] : 0.0f;
    }
    const float knownscale = ws_known ? ws[n] : 0.0f;
    auto value_of = [&](u32 code, float s, float z, int gbase) {
        if (p.L) return srow[gbase + (int)code];  // codebook: entry c of the table is levels[n][g][c] (dequant16)
        float x;
        if (p.fmt.kind == SDNQ_KIND_INT) x = (float)((int)code - 8);
        else if (p.fmt.kind == SDNQ_KIND_UINT) x = (float)code;
        else x = decode_exmy(code, p.fmt.ebits, p.fmt.mbits, p.fmt.kind == SDNQ_KIND_UFLOAT);
        float v = zrow ? fmaf(x, s, z) : x * s;  // dequant16
        if (p.sdt != SDNQ_F32) v = round_rt(v, p.sdt);
        return v;
    };
    const int quad = lane & 3;
    float scale = knownscale;
    if (!ws_known) {
        // amax over the row = max over (group, code present) of |value|: the four lanes of a group each test four codes against
        // the codes that actually occur in their 16 elements
        float amax = 0.0f;
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const bool live = (int64_t)ps * 1024 + lane * 16 < p.K;
            u32 present = 0;  // bit c set: code c occurs among this lane's 16 elements
#pragma unroll
            for (int j = 0; j < 8; ++j) present |= (1u << ((cw[ps].x >> (4 * j)) & 15u)) | (1u << ((cw[ps].y >> (4 * j)) & 15u));
            if (!live) present = 0;
            // union over the quad (the table entries are split by code, the occurrences by lane)
            present |= (u32)__builtin_amdgcn_update_dpp(0, (int)present, 0xB1, 0xf, 0xf, false);
            present |= (u32)__builtin_amdgcn_update_dpp(0, (int)present, 0x4E, 0xf, 0xf, false);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const u32 code = 4u * quad + e;
                const float v = fabsf(value_of(code, sg[ps], zg[ps], gb[ps]));
                if ((present >> code) & 1u) amax = fmaxf(amax, v);
            }
        }
        amax = wave_max(amax);
        const float qmax = (MM == SDNQ_MM_I8) ? 127.0f : 448.0f;
        scale = round_rt(amax / qmax, p.sdt);
        if (lane == 0) ws[n] = scale;
    }
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        const int64_t k0 = (int64_t)ps * 1024 + lane * 16;
        // this lane's four table entries: codes 4 * quad .. 4 * quad + 3 (the expression of requant_kernel's second pass)
        u32 mine = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = value_of(4u * quad + e, sg[ps], zg[ps], gb[ps]);
            u32 byte;
            if constexpr (MM == SDNQ_MM_I8) {
                float q = __builtin_rintf(round_rt(v / scale, p.sdt));
                if (q != q) q = 0.0f;  // 0/0 of a constant row: NaN.to(int8) is 0 in the reference
                q = fminf(fmaxf(q, -128.0f), 127.0f);
                byte = (u32)(int)q & 0xffu;
            } else {
                float q = round_rt(v / scale, p.sdt);
                if (q != q) q = 0.0f;
                q = fminf(fmaxf(q, -448.0f), 448.0f);
                byte = f32_to_e4m3fn_clamped(q);
            }
            mine |= byte << (8 * e);
        }
        // sdnq_hip_lut4_build (round 6: the GEMM that expands the codes itself, gemm_w4.hip): the tables ARE the result -- lane l's four
        // entries are dword (l & 3) of the table of (row n, columns 64 (l >> 2) ..), i.e. lut[n][K / 64][16 bytes] written lane-linearly
        if (lut != nullptr) {
            if (k0 < p.K) lut[(n * p.K + k0) >> 4] = mine;
            continue;
        }
        // the quad's four dwords = the 16-entry table (entry c in byte c & 3 of dword c >> 2)
        const u32 t0 = (u32)__builtin_amdgcn_update_dpp(0, (int)mine, 0x00, 0xf, 0xf, false);  // quad_perm [0,0,0,0]
        const u32 t1 = (u32)__builtin_amdgcn_update_dpp(0, (int)mine, 0x55, 0xf, 0xf, false);  // [1,1,1,1]
        const u32 t2 = (u32)__builtin_amdgcn_update_dpp(0, (int)mine, 0xAA, 0xf, 0xf, false);  // [2,2,2,2]
        const u32 t3 = (u32)__builtin_amdgcn_update_dpp(0, (int)mine, 0xFF, 0xf, 0xf, false);  // [3,3,3,3]
        u32 o[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const u32 half = ((h < 2 ? cw[ps].x : cw[ps].y) >> (16 * (h & 1))) & 0xffffu;  // 4 codes: element j = nibble j
            const u32 a = __builtin_amdgcn_perm(0u, half, 0x01010000u);            // bytes [b0, b0, b1, b1]
            const u32 sel = (a & 0x000f000fu) | ((a >> 4) & 0x0f000f00u);          // one code per byte
            const u32 lo = __builtin_amdgcn_perm(t1, t0, sel & 0x07070707u);       // entries 0..7 (selector k = byte k of {t1:t0})
            const u32 hi = __builtin_amdgcn_perm(t3, t2, sel & 0x07070707u);       // entries 8..15
            const u32 m = ((sel >> 3) & 0x01010101u) * 0xffu;                      // 0xff where the code is >= 8
            o[h] = (hi & m) | (lo & ~m);
        }
        if (k0 < p.K) *(uint4*)(wq + n * p.K + k0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// float16 matmul operand straight from stored FLOAT codes (round 6, linear_fp16.py:27-31: `unpack_float(...).to(float16)` for packed
// formats, `weight.to(float16)` for native fp8): the decoded value rounded to float16 (exact for every format of <= 11 significand bits)
__global__ __launch_bounds__(256) void unpack_mm_f16_kernel(const DeqParams p, uint16_t* __restrict__ wq) {
    const int64_t units = p.N * p.K / 16;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    float v[16];
    load16_values(p.w, u * 16, p.fmt, v);
    *(uint4*)(wq + u * 16) = Vec16<SDNQ_F16>::pack(v);
    *(uint4*)(wq + u * 16 + 8) = Vec16<SDNQ_F16>::pack(v + 8);
}

// matmul operand straight from the stored codes (no scaling): see sdnq_hip_unpack_mm in the header
template <int MM>
__global__ __launch_bounds__(256) void unpack_mm_kernel(const DeqParams p, uint8_t* __restrict__ wq) {
    const int64_t units = p.N * p.K / 16;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    float v[16];
    load16_values(p.w, u * 16, p.fmt, v);
    u32 o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        u32 byte;
        if constexpr (MM == SDNQ_MM_I8) {
            int iv = (int)v[j];  // exact: |v| < 256
            if (p.fmt.kind == SDNQ_KIND_UINT && p.fmt.storage == SDNQ_ST_RAW8) iv ^= 0x80;  // uint8 -> int8 (linear_int8.py:46)
            byte = (u32)iv & 0xffu;
        } else {
            byte = f32_to_e4m3fn(v[j]);
        }
        o[j >> 2] |= byte << (8 * (j & 3));
    }
    *(uint4*)(wq + u * 16) = make_uint4(o[0], o[1], o[2], o[3]);
}

// The (output, SVD) dtype pairs dequant_kernel and embedding_kernel are built for: equal, or one of the two float32.  f(O, S) as
// dispatch_int calls it; false for any other pair.
template <typename F>
bool dispatch_out_svd(int out_t, int svd_t, F&& f) {
    return dispatch_float(out_t, [&](auto O) {
        return dispatch_float(svd_t, [&](auto S) {
            if constexpr (O.value == SDNQ_F32 || S.value == SDNQ_F32 || O.value == S.value) return f(O, S);
            return false;
        });
    });
}

}  // namespace

extern "C" int sdnq_hip_dequant(const SdnqWeight* w, int hadamard_group, void* out, int out_dtype, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!out) return SDNQ_ERR_NULL;
    if (out_dtype < 0 || out_dtype > 2) return SDNQ_ERR_DTYPE;
    if ((uintptr_t)out % 16) return SDNQ_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t units = p.N * (p.K / 16);
    dim3 grid((unsigned)((units + 255) / 256)), block(256);
    const int svd_t = p.svd_up ? w->svd_dtype : out_dtype;
    if (!dispatch_out_svd(out_dtype, svd_t, [&](auto O, auto S) {
            hipLaunchKernelGGL((dequant_kernel<O.value, S.value>), grid, block, 0, s, p, out);
            return true;
        }))
        return SDNQ_ERR_DTYPE;
    SDNQ_CHECK_LAUNCH();
    if (hadamard_group != 0) return sdnq_hip_hadamard(out, out_dtype, p.N, p.K, p.K, hadamard_group, out, p.K, stream);
    return SDNQ_OK;
}

extern "C" int sdnq_hip_embedding(const SdnqWeight* w, int hadamard_group, const void* ids, int ids_dtype, int64_t n_ids,
                                  int has_embed_scale, double embed_scale, void* out, int out_dtype, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (w->positions > 1) return SDNQ_ERR_SHAPE;
    if (!out || (!ids && n_ids > 0)) return SDNQ_ERR_NULL;
    if (out_dtype < 0 || out_dtype > 2 || (ids_dtype != SDNQ_IDS_I32 && ids_dtype != SDNQ_IDS_I64)) return SDNQ_ERR_DTYPE;
    if (n_ids < 0) return SDNQ_ERR_SHAPE;
    const int log2g = hadamard_log2(hadamard_group, p.K);
    if (log2g < 0) return SDNQ_ERR_SHAPE;
    if ((uintptr_t)out % 16 || (p.svd_up && (uintptr_t)p.svd_down % 16)) return SDNQ_ERR_ALIGN;
    if (n_ids == 0) return SDNQ_OK;
    const int64_t waves = n_ids * ((p.K + 1023) / 1024);
    if ((waves + 3) / 4 > 0x7fffffff) return SDNQ_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    const int svd_t = p.svd_up ? w->svd_dtype : out_dtype;
    const int ids64 = ids_dtype == SDNQ_IDS_I64;
    const float es = (float)embed_scale;  // a Python float multiplies in the tensor's op-math type (float32 for 16-bit and f32 tensors)
    if (!dispatch_out_svd(out_dtype, svd_t, [&](auto O, auto S) {
            hipLaunchKernelGGL((embedding_kernel<O.value, S.value>), grid, block, 0, s, p, ids, ids64, n_ids, log2g, has_embed_scale, es, out);
            return true;
        }))
        return SDNQ_ERR_DTYPE;
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int64_t sdnq_hip_dequant_loss_workspace_bytes(int64_t n, int64_t k) {
    if (n <= 0 || k <= 0) return SDNQ_ERR_SHAPE;
    return loss_blocks(n, k) * (int64_t)sizeof(double);
}

extern "C" int sdnq_hip_dequant_loss(const SdnqWeight* w, int hadamard_group, const void* ref, int ref_dtype, int64_t ld_ref,
                                     double* sum_out, void* workspace, int64_t workspace_bytes, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!ref || !sum_out || !workspace) return SDNQ_ERR_NULL;
    if (ref_dtype < 0 || ref_dtype > 2) return SDNQ_ERR_DTYPE;
    if (ld_ref < p.K) return SDNQ_ERR_SHAPE;
    const int log2g = hadamard_log2(hadamard_group, p.K);
    if (log2g < 0) return SDNQ_ERR_SHAPE;
    const int rb = ref_dtype == SDNQ_F32 ? 4 : 2;
    if ((uintptr_t)ref % 16 || (ld_ref * rb) % 16 || (uintptr_t)sum_out % 8 || (uintptr_t)workspace % 8 || (p.svd_up && (uintptr_t)p.svd_down % 16))
        return SDNQ_ERR_ALIGN;
    const int64_t blocks = loss_blocks(p.N, p.K);
    if (workspace_bytes < blocks * (int64_t)sizeof(double)) return SDNQ_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int svd_t = p.svd_up ? w->svd_dtype : SDNQ_F32;
    double* part = (double*)workspace;
    dim3 grid((unsigned)blocks), block(256);
    const bool built = dispatch_float(ref_dtype, [&](auto R) {  // every (reference, SVD) dtype pair
        return dispatch_float(svd_t, [&](auto S) {
            hipLaunchKernelGGL((dequant_loss_kernel<R.value, S.value>), grid, block, 0, s, p, ref, ld_ref, log2g, part);
            return true;
        });
    });
    if (!built) return SDNQ_ERR_DTYPE;
    SDNQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)part, blocks, sum_out);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

// 4-bit packed weights in groups of a multiple of 64 go through the table kernel (bit-identical, ~2-3x fewer vector instructions);
// `ws_known` (row scales already in ws) is honoured by it and ignored -- the scales are simply recomputed -- by the general kernel
static int launch_requant(const DeqParams& p, int mm_dtype, void* wq, float* ws, int ws_known, hipStream_t s, void* lut = nullptr) {
    dim3 grid((unsigned)((p.N + 3) / 4)), block(256);
    // test / tuning aid, read per call (a re-quantization is a whole-weight pass: a getenv is nothing beside it) so that one
    // process can A/B the table kernel against the general one (tests/test_gpu_parity.py)
    const char* lut_env = getenv("SDNQ_HIP_REQUANT_LUT");
    const bool no_lut = lut_env && atoi(lut_env) == 0;
    const bool lut_ok = p.fmt.storage == SDNQ_ST_PACKED_U8 && p.fmt.bits == 4 && p.P == 1 && (p.group_size % 64) == 0 && (p.K % 64) == 0 && !p.fmt.native_float;
    const bool use_lut = lut_ok && (!no_lut || lut != nullptr);
    const int np = (int)((p.K + 1023) / 1024);
    if (lut != nullptr && !(lut_ok && np <= 16)) return SDNQ_ERR_UNSUPPORTED;  // tables exist for what the table kernel handles
    const int np_built = np <= 6 ? np : (np <= 8 ? 8 : (np <= 12 ? 12 : 16));  // the table kernel's passes per row: 1..6 exactly, then 8, 12, 16
    const bool built = dispatch_int<SDNQ_MM_I8, SDNQ_MM_FP8>(mm_dtype, [&](auto MM) {
        if (!(use_lut && np <= 16)) {
            hipLaunchKernelGGL((requant_kernel<MM.value>), grid, block, 0, s, p, (uint8_t*)wq, ws, (float*)nullptr);
            return true;
        }
        return dispatch_int<1, 2, 3, 4, 5, 6, 8, 12, 16>(np_built, [&](auto NP) {
            hipLaunchKernelGGL((requant_lut4_kernel<MM.value, NP.value>), grid, block, 0, s, p, (uint8_t*)wq, ws, ws_known, (u32*)lut);
            return true;
        });
    });
    if (!built) return SDNQ_ERR_DTYPE;
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_requant(const SdnqWeight* w, int mm_dtype, void* wq, float* ws, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!wq || !ws) return SDNQ_ERR_NULL;
    if ((uintptr_t)wq % 16) return SDNQ_ERR_ALIGN;
    p.svd_up = nullptr; p.svd_down = nullptr;  // re_quantize_matmul never receives the SVD factors (linear_int8.py:105)
    hipStream_t s = (hipStream_t)stream;
    return launch_requant(p, mm_dtype, wq, ws, 0, s);
}

extern "C" int sdnq_hip_requant_ws(const SdnqWeight* w, int mm_dtype, void* wq, float* ws, int ws_known, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!wq || !ws) return SDNQ_ERR_NULL;
    if ((uintptr_t)wq % 16) return SDNQ_ERR_ALIGN;
    p.svd_up = nullptr; p.svd_down = nullptr;
    return launch_requant(p, mm_dtype, wq, ws, ws_known, (hipStream_t)stream);
}

extern "C" int sdnq_hip_lut4_build(const SdnqWeight* w, int mm_dtype, float* ws, int ws_known, void* lut, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!ws || !lut) return SDNQ_ERR_NULL;
    if ((uintptr_t)lut % 16) return SDNQ_ERR_ALIGN;
    p.svd_up = nullptr; p.svd_down = nullptr;  // as sdnq_hip_requant
    return launch_requant(p, mm_dtype, nullptr, ws, ws_known, (hipStream_t)stream, lut);
}

extern "C" int sdnq_hip_requant_asym(const SdnqWeight* w, void* wq, float* ws, float* wzp, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!wq || !ws || !wzp) return SDNQ_ERR_NULL;
    if ((uintptr_t)wq % 16) return SDNQ_ERR_ALIGN;
    p.svd_up = nullptr; p.svd_down = nullptr;  // as sdnq_hip_requant (linear_uint8.py:110)
    // (16-bit scales: get_scale_asymmetric and the quotient round in the scale dtype, see requant_kernel)
    dim3 grid((unsigned)((p.N + 3) / 4)), block(256);
    hipLaunchKernelGGL((requant_kernel<SDNQ_MM_I8, true>), grid, block, 0, (hipStream_t)stream, p, (uint8_t*)wq, ws, wzp);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_unpack_mm(const SdnqWeight* w, int mm_dtype, void* wq, sdnq_stream_t stream) {
    DeqParams p{};
    int st = fill_params(w, p);
    if (st != SDNQ_OK) return st;
    if (!wq) return SDNQ_ERR_NULL;
    if ((uintptr_t)wq % 16) return SDNQ_ERR_ALIGN;
    if (mm_dtype == SDNQ_MM_I8) {
        if ((p.fmt.kind != SDNQ_KIND_INT && p.fmt.kind != SDNQ_KIND_UINT) || p.fmt.bits > 8) return SDNQ_ERR_DTYPE;
    } else if (mm_dtype == SDNQ_MM_FP8) {
        if (p.fmt.kind != SDNQ_KIND_FLOAT || p.fmt.bits > 8) return SDNQ_ERR_DTYPE;
    } else if (mm_dtype == SDNQ_MM_F16) {
        if (p.fmt.kind != SDNQ_KIND_FLOAT || p.fmt.bits > 16) return SDNQ_ERR_DTYPE;
    } else {
        return SDNQ_ERR_DTYPE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t units = p.N * p.K / 16;
    dim3 grid((unsigned)((units + 255) / 256)), block(256);
    if (mm_dtype == SDNQ_MM_F16) {
        hipLaunchKernelGGL(unpack_mm_f16_kernel, grid, block, 0, s, p, (uint16_t*)wq);
        SDNQ_CHECK_LAUNCH();
        return SDNQ_OK;
    }
    if (mm_dtype == SDNQ_MM_I8) hipLaunchKernelGGL((unpack_mm_kernel<SDNQ_MM_I8>), grid, block, 0, s, p, (uint8_t*)wq);
    else hipLaunchKernelGGL((unpack_mm_kernel<SDNQ_MM_FP8>), grid, block, 0, s, p, (uint8_t*)wq);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
