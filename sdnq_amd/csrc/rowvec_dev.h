// How the one-wave-per-row kernels move a row: 8 consecutive elements per lane per 512-element pass, every global access a 16-byte
// (bf16 / f16) or 2 x 16-byte (f32) lane-contiguous vector.  Shared by the row quantizers (rowquant.hip) and the fused
// normalisation + row quantization (normquant.hip); the per-element quantizer arithmetic both apply is quant8_dev.h.  (The row
// quantizer's write-through code store and prefetch workgroups stay written out in rowquant_kernel: called from here, one
// instantiation's register allocation and the prefetch block's operand order changed -- profiles/normquant_kernel_compare.txt.)
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
