// The rotated fused producers (normquant_had.hip, actquant_had.hip): a norm or an activation writes y and, in the same launch, the int8 /
// fp8 codes and row scale of the Hadamard-ROTATED y -- what sdnq_hip_rowquant(y, mm, hadamard_group) writes for that y, bit for bit.
// Here: the two kernel skeletons.  What a row is and how its y comes about (statistics, norm8 / act8: the plain producers' own code,
// normquant_dev.h / actquant_dev.h) is a ROW type:
//   ROW::Args (by-value kernel argument: M, y, xq, xs, log2g and the operands), ROW::T (row dtype), ROW::len(A) (row length),
//   row.begin(A, m, k0, lane)  the row's loads (NP > 0: the NP passes from element k0 on, all in flight) and statistics,
//   row.y8(p, idx, ok)         the rounded y of this lane's 8 elements at idx = k0 + 512 p + 8 lane, packed as it is stored (zeros past the end).
//
// producer_had256_kernel: group 256 on 16-bit rows, the row quantizer's matrix-core rotation (rowquant_had256_kernel; had256_group).
//   The producers hold a pass as 8 consecutive elements per lane (their statistics are summed in that layout, so it cannot change);
//   had256_group wants 4 consecutive elements per lane, 16 (lane & 15) + 4 (lane >> 4) of each group.  The re-layout goes through a
//   wave-private LDS tile, one 512-element pass (1 KB) at a time: a lane writes its 16-byte vector and reads two 8-byte pieces, one per
//   group.  CHOSEN OVER an in-register re-layout: a lane's 4 elements of a group come from lane 2 (l & 15) + (l >> 5) of the pass, a
//   permutation over all six lane bits -- four ds_bpermute per pass (each an LDS-crossbar round trip, what lane_xor avoids) plus the
//   selects, against one ds_write_b128 and two ds_read_b64 here.  (Neither form is measured against the other.)
//   Banks: the write is lane-contiguous.  A read's rows of 32 bytes would put rows r and r + 8 on the same 8 banks; every 256-byte
//   quarter of the tile is shifted by 16 bytes more than the one before, so the 32 lanes of a read half touch 64 different banks.
//   No workgroup barrier: a row never leaves its wave, and LDS runs a wave's instructions in order (wave_lds_sync holds the compiler to
//   the program order).  The rotated row stays packed two to a register (2 registers per group) between amax and the codes.
//   NP > 0, WPR == 1: a row per wave, four rows per workgroup, K <= NP * 512 <= 4096.
//   NP > 0, WPR == 4: the row over the four waves of the workgroup, NP passes each, the partial amax meeting in LDS (one barrier) --
//       rows whose y needs no statistics (activations), K <= 16384.
//   NP == 0: the sweep form -- y and the rotation computed twice, once for amax and once for the codes (same inputs, same operations:
//       the same bits); rows with statistics past 4096.
// producer_fwht_kernel: every other group (and 256 past 16384): wave_hadamard on the pass in registers between the y store and the amax,
//   exactly where rowquant_kernel<..., HAD = true> has it; no LDS.  NP > 0: the rotated row packed in registers; NP == 0: computed twice.
#pragma once
#include "hadamard_dev.h"
#include "quant8_dev.h"
#include "rowvec_dev.h"
#include "sdnq_dev.h"

constexpr int HAD_TILE_BYTES = 1024 + 4 * 16;  // a pass and the quarters' shifts

__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// a pass as lane vectors (8 consecutive elements per lane) -> its two groups as had256_group's operand (4 consecutive elements per lane)
__device__ __forceinline__ void pass_to_groups(char* tile, int lane, const uint4& yp, uint2 (&raw)[2]) {
    wave_lds_sync();  // (the reads of the pass before are behind us)
    *(uint4*)(tile + 16 * lane + 16 * (lane >> 4)) = yp;
    wave_lds_sync();
    const int off = 32 * (lane & 15) + 8 * (lane >> 4) + 16 * ((lane & 15) >> 3);
    raw[0] = *(const uint2*)(tile + off);
    raw[1] = *(const uint2*)(tile + off + 512 + 32);
}

// element `hi` (0 / 1) of a dword of two 16-bit activations, as a float
template <int T_ID> __device__ __forceinline__ float unpk16(u32 w, int hi) {
    if constexpr (T_ID == SDNQ_BF16) return __uint_as_float(hi ? (w & 0xffff0000u) : (w << 16));
    else return f16_bits_to_f32((uint16_t)(hi ? (w >> 16) : (w & 0xffffu)));
}

// 4-byte store of codes, write-through as store_codes8 (rowvec_dev.h)
__device__ __forceinline__ void store_codes4_wt(uint8_t* dst, u32 w) {
#if !defined(SDNQ_RQ_STORE_PLAIN)
    asm volatile("global_store_dword %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(w) : "memory");
#else
    *(u32*)dst = w;
#endif
}

// The codes of a lane's 4 rotated elements of a group (p0, p1: packed pairs), the arithmetic of rowquant_had256_kernel's two loops.
// COPIES, with unpk16 and store_codes4_wt above: called from rowquant_had256_kernel in place of its written-out loops, these helpers
// changed the listing of all 24 of its instantiations (register allocation; +-15 instructions in six), and that kernel's code is held
// fixed.  What keeps the copies in step are the bit-equality tests (tests/test_producer_hadamard_gpu.py: lean int8, general int8 on
// the zero row, fp8).  The lean int8 codes where the scale is `fast` ...
template <int T_ID>
__device__ __forceinline__ u32 had256_codes_lean(u32 p0, u32 p1, const RowDiv& rd) {
    asm volatile("" : "+v"(p0), "+v"(p1));  // (opaque, as there: the unpacking of every group is otherwise hoisted above the branch)
    const pv2f a = {unpk16<T_ID>(p0, 0), unpk16<T_ID>(p0, 1)}, b = {unpk16<T_ID>(p1, 0), unpk16<T_ID>(p1, 1)};
    return pack4_rne_i8(fastdiv2(a, rd), fastdiv2(b, rd));
}
// ... and the general ones (scale 0 / inf / nan / extreme; fp8 with the clamp)
template <int T_ID, int MM>
__device__ __forceinline__ u32 had256_codes(u32 p0, u32 p1, const RowDiv& rd) {
    float qd[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ve = unpk16<T_ID>(e < 2 ? p0 : p1, e & 1);
        qd[e] = rd.fast ? rd.fastdiv(ve) : ve / rd.scale;  // rd.fast is wave-uniform
    }
    if constexpr (MM == SDNQ_MM_FP8) {
        float c[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float q = qd[e];
            if (q != q) q = 0.0f;
            c[e] = fminf(fmaxf(q, -448.0f), 448.0f);
        }
        return pack4_e4m3fn_clamped(c[0], c[1], c[2], c[3]);
    } else {
        u32 w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float q = (rd.scale == 0.0f) ? 0.0f : __builtin_rintf(qd[e]);
            q = fminf(fmaxf(q, -128.0f), 127.0f);
            w |= ((u32)(int)q & 0xffu) << (8 * e);
        }
        return w;
    }
}

template <class ROW, int MM, int NP, int WPR>
__global__ __launch_bounds__(256) void producer_had256_kernel(const typename ROW::Args A) {
    constexpr int T_ID = ROW::T;
    static_assert(WPR == 1 || (WPR == 4 && NP > 0), "a row per wave, or the row over the four waves in registers");
    __shared__ __attribute__((aligned(16))) char s_tile[4][HAD_TILE_BYTES];
    __shared__ float s_amax[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t m = WPR == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    if (WPR == 1 && m >= A.M) return;  // whole wave exits together (WPR == 4: one row per workgroup, every wave reaches the barrier)
    const int64_t K = ROW::len(A);
    const int64_t k0 = WPR == 1 ? 0 : (int64_t)wv * NP * 512;  // first element of this wave's part
    const int64_t npass = NP > 0 ? NP : (K + 511) / 512;
    constexpr int UNR = NP > 0 ? NP : 1;
    char* tile = s_tile[wv];
    float hf[4];
    had16_operand(lane, hf);
    ROW row;
    row.begin(A, m, k0, lane);
    void* yrow = A.y ? (char*)A.y + m * K * 2 : nullptr;
    // pass p of this wave: y (stored on the `first` sweep) and its two rotated groups, rounded and packed (a group past the end: zeros)
    auto rotated = [&](int64_t p, bool first, u32 (&g)[2][2]) {
        const int64_t base = k0 + p * 512, idx = base + lane * 8;
        const bool ok = idx < K;
        const uint4 yp = row.y8(p, idx, ok);
        if (first && yrow && ok) *(uint4*)((uint16_t*)yrow + idx) = yp;
        g[0][0] = g[0][1] = g[1][0] = g[1][1] = 0u;
        if (base < K) {  // wave-uniform
            uint2 raw[2];
            pass_to_groups(tile, lane, yp, raw);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (base + 256 * h < K) {  // wave-uniform (K % 256 == 0)
                    const v4f r = had256_group<T_ID>(raw[h], hf);
                    g[h][0] = pack2<T_ID>(r[0], r[1]);
                    g[h][1] = pack2<T_ID>(r[2], r[3]);
                }
            }
        }
    };
    u32 pk[NP > 0 ? NP : 1][2][2];
    float amax = 0.0f;
#pragma unroll UNR
    for (int64_t p = 0; p < npass; ++p) {
        u32 g[2][2];
        rotated(p, true, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(unpk16<T_ID>(g[e >> 2][(e >> 1) & 1], e & 1)));
        if constexpr (NP > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[p][e >> 1][e & 1] = g[e >> 1][e & 1];
        }
    }
    amax = wave_max(amax);
    if constexpr (WPR > 1) {
        if (lane == 0) s_amax[wv] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(s_amax[0], s_amax[1]), fmaxf(s_amax[2], s_amax[3]));
    }
    const float scale = amax / ((MM == SDNQ_MM_I8) ? 127.0f : 448.0f);  // IEEE division, as rowquant_had256_kernel
    if (lane == 0 && (WPR == 1 || wv == 0)) A.xs[m] = scale;
    RowDiv rd;
    rd.set(scale);
    uint8_t* qrow = A.xq + m * K + k0 + 16 * (lane & 15) + 4 * (lane >> 4);  // this lane's 4 codes of the wave's first group
    // the packed groups of pass p again: from the registers, or computed once more
    auto groups = [&](int64_t p, u32 (&g)[2][2]) {
        if constexpr (NP > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e >> 1][e & 1] = pk[p][e >> 1][e & 1];
        } else {
            rotated(p, false, g);
        }
    };
    if (MM == SDNQ_MM_I8 && rd.fast) {  // wave-uniform
#pragma unroll UNR
        for (int64_t p = 0; p < npass; ++p) {
            u32 g[2][2];
            groups(p, g);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (k0 + p * 512 + 256 * h < K) store_codes4_wt(qrow + p * 512 + 256 * h, had256_codes_lean<T_ID>(g[h][0], g[h][1], rd));
        }
    } else {
#pragma unroll UNR
        for (int64_t p = 0; p < npass; ++p) {
            u32 g[2][2];
            groups(p, g);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (k0 + p * 512 + 256 * h < K) store_codes4_wt(qrow + p * 512 + 256 * h, had256_codes<T_ID, MM>(g[h][0], g[h][1], rd));
        }
    }
}

template <class ROW, int MM, int NP>
__global__ __launch_bounds__(256) void producer_fwht_kernel(const typename ROW::Args A) {
    constexpr int T_ID = ROW::T;
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= A.M) return;  // whole wave exits together
    const int64_t K = ROW::len(A);
    const int64_t npass = NP > 0 ? NP : (K + 511) / 512;
    constexpr int UNR = NP > 0 ? NP : 1;
    const float hscale = hadamard_scale(A.log2g, T_ID);
    ROW row;
    row.begin(A, m, 0, lane);
    void* yrow = A.y ? (char*)A.y + m * K * 2 : nullptr;
    // pass p: y (stored on the `first` sweep), rotated and rounded to the row dtype as rowquant_kernel does it
    auto rotated = [&](int64_t p, bool first, float (&t)[8]) {
        const int64_t idx = p * 512 + lane * 8;
        const bool ok = idx < K;
        const uint4 yp = row.y8(p, idx, ok);
        if (first && yrow && ok) *(uint4*)((uint16_t*)yrow + idx) = yp;
        Vec16<T_ID>::unpack(yp, t);
        if (p * 512 < K) {  // wave-uniform
            wave_hadamard(t, A.log2g, hscale);
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] = FT<T_ID>::round(t[e]);
        }
    };
    uint4 rp[NP > 0 ? NP : 1];
    float amax = 0.0f;
#pragma unroll UNR
    for (int64_t p = 0; p < npass; ++p) {
        float t[8];
        rotated(p, true, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(t[e]));
        if constexpr (NP > 0) rp[p] = Vec16<T_ID>::pack(t);  // (rounded already: exact)
    }
    RowDiv rd;
    rd.set(row_scale<MM>(amax, lane, A.xs + m));
    uint8_t* qrow = A.xq + m * K;
    int isum = 0;  // (quant8's row sum: unused here)
#pragma unroll UNR
    for (int64_t p = 0; p < npass; ++p) {
        const int64_t idx = p * 512 + lane * 8;
        float t[8];
        if constexpr (NP > 0) Vec16<T_ID>::unpack(rp[p], t);
        else rotated(p, false, t);
        if (idx < K) store_codes8(qrow + idx, quant8<MM>(t, rd, isum));
    }
}
