// How the one-wave-per-row kernels move a row: 8 consecutive elements per lane per 512-element pass, every global access a 16-byte
// (bf16 / f16) or 2 x 16-byte (f32) lane-contiguous vector.  Shared by the row quantizers (rowquant.hip), the fused normalisation + row
// quantization (normquant.hip) and the fused activation + row quantization (actquant.hip); the per-element quantizer arithmetic all of
// them apply is quant8_dev.h.  The write-through code store, the prefetch workgroups and the row scale at the end of this file serve
// normquant.hip and actquant.hip.  (The row quantizer's own stay written out in rowquant_kernel: called from here, one instantiation's
// register allocation and the prefetch block's operand order changed -- profiles/normquant_kernel_compare.txt.)
#pragma once
#include "sdnq_dev.h"

// 8 consecutive elements of a row as floats; lanes past the end of the row (`ok` false) get zeros.  The load itself is
// UNCONDITIONAL (a lane past the end re-reads the start of its row): a load under `if (ok)` makes the compiler close every
// pass with its own s_waitcnt vmcnt(0), so the passes of a row were fetched one HBM round trip after the other (round 1:
// 12.2 us for 1024 x 5120 rows, 8.9 us with the loads in flight together).
template <int T_ID>
__device__ __forceinline__ void load8_raw(const void* row, int64_t idx, bool ok, uint4& a, uint4& b) {
    const int64_t i = ok ? idx : 0;
    if constexpr (T_ID == SDNQ_F32) {
        a = *(const uint4*)((const float*)row + i);
        b = *(const uint4*)((const float*)row + i + 4);
    } else {
        a = *(const uint4*)((const uint16_t*)row + i);
        b = a;
    }
}
template <int T_ID>
__device__ __forceinline__ void unpack8(const uint4& a, const uint4& b, bool ok, float (&v)[8]) {
    if constexpr (T_ID == SDNQ_F32) {
        Vec16<SDNQ_F32>::unpack(a, v);
        Vec16<SDNQ_F32>::unpack(b, v + 4);
    } else {
        Vec16<T_ID>::unpack(a, v);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ok ? v[e] : 0.0f;
}
template <int T_ID>
__device__ __forceinline__ void load8(const void* row, int64_t idx, bool ok, float (&v)[8]) {
    uint4 a, b;
    load8_raw<T_ID>(row, idx, ok, a, b);
    unpack8<T_ID>(a, b, ok, v);
}

template <int T_ID>
__device__ __forceinline__ void store8(void* row, int64_t idx, const float (&v)[8]) {
    if constexpr (T_ID == SDNQ_F32) {
        *(uint4*)((float*)row + idx) = Vec16<SDNQ_F32>::pack(v);
        *(uint4*)((float*)row + idx + 4) = Vec16<SDNQ_F32>::pack(v + 4);
    } else {
        *(uint4*)((uint16_t*)row + idx) = Vec16<T_ID>::pack(v);
    }
}

// 8-byte store of quantized codes, write-through (sc0 sc1) as rowquant_kernel's: the codes are read by the following GEMM from OTHER
// XCDs; left dirty in this XCD's L2 they cost that GEMM a remote write-back per first touch
__device__ __forceinline__ void store_codes8(uint8_t* dst, const uint2& qv) {
#if !defined(SDNQ_RQ_STORE_PLAIN)
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const v2i_t w2 = {(int)qv.x, (int)qv.y};
    asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(w2) : "memory");
#else
    *(uint2*)dst = qv;
#endif
}

// software prefetch of a following GEMM's weight operand, as rowquant_kernel's: workgroups appended behind a launch's row blocks stream
// it once into the last-level cache.  The entry points of normquant.hip / actquant.hip take no such operand (pf_vecs is 0, no workgroup
// is appended): the leading branch of their kernels is never taken.  It stays because the kernels measured slower without it in 6 of
// 33 cases (profiles/producer_refactor_bench.jsonl, build "operand_removed"; that build also held the wave index in an SGPR, so what
// the plain removal costs is not measured).  `block`: index among those workgroups (THREADS threads each); `sink`: any float the kernel
// may write (the store never happens: it keeps the loads alive).
template <int THREADS = 256>
__device__ __forceinline__ void prefetch_block(const uint4* __restrict__ pf, int64_t pf_vecs, int64_t block, float* sink) {
    const int64_t base = block * (THREADS * 8) + threadIdx.x;
    u32 acc = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int64_t i = base + (int64_t)u * THREADS;
        if (i < pf_vecs) { const uint4 v = pf[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
    }
    if (acc == 0x9e3779b9u && pf_vecs < 0) sink[0] = 0.0f;  // never true: keeps the loads alive
}

// the scale of a row whose wave holds per-lane maxima of |y|: amax / qmax of the MM codes, stored by lane 0, returned to every lane
template <int MM>
__device__ __forceinline__ float row_scale(float amax, int lane, float* xs) {
    amax = wave_max(amax);
    const float scale = amax / ((MM == SDNQ_MM_I8) ? 127.0f : 448.0f);  // IEEE division, as rowquant_kernel
    if (lane == 0) *xs = scale;
    return scale;
}
