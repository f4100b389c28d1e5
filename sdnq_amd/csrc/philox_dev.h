// The project's one random-number generator on the device, shared by the units that draw from it (optim.hip: stochastic rounding and the
// noise of stochastic uint8 state; linear_float.hip and lowrank_train.hip: the dropout mask of the adapter kernels).
//
// Philox4x32-10, key = seed, counter = (e8 low, e8 high | stream << 28, offset low, offset high) with e8 = (logical element index) / 8:
// one call yields four 32-bit words = 16 bits for each of 8 consecutive elements, element e taking half e & 1 of word (e % 8) >> 1.  The
// bits an element gets depend on (seed, offset, stream, element index) alone, not on the launch geometry or on a row stride.
// Streams: 0 parameter, 1 exp_avg, 2 exp_avg_sq, 3 and 4 the second calls behind the normals of stochastic uint8 state (optim.hip);
// 5 the dropout mask of the adapter kernels.
#pragma once
#include "sdnq_dev.h"

namespace {

__device__ __forceinline__ uint4 aw_philox(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// ---- dropout on a 16-byte chunk of 16-bit elements --------------------------------------------------------------------------------------
// An element is KEPT iff its 16 random bits are >= thr (1 <= thr <= 65535: the probability of a drop is thr / 65536).  The survivors are
// not rescaled here: 1 / (1 - p) travels in the float32 scale the adapter kernels already take.
constexpr u32 PHILOX_STREAM_DROPOUT = 5;

struct DropArgs {
    u32 thr, seed_lo, seed_hi, off_lo, off_hi;
};

__device__ __forceinline__ uint4 dropout_words(int64_t e8, const DropArgs& d) {
    return aw_philox((u32)e8, (u32)((uint64_t)e8 >> 32) | (PHILOX_STREAM_DROPOUT << 28), d.off_lo, d.off_hi, d.seed_lo, d.seed_hi);
}

// m[c]: all ones in the 16-bit halves of dword c whose elements are kept (element 2 c is the low half of dword c), for the 8 elements
// with logical indices 8 e8 .. 8 e8 + 7
__device__ __forceinline__ void dropout_masks(int64_t e8, const DropArgs& d, u32 (&m)[4]) {
    const uint4 r = dropout_words(e8, d);
    const u32 w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) m[c] = ((w[c] & 0xffffu) >= d.thr ? 0xffffu : 0u) | ((w[c] >> 16) >= d.thr ? 0xffff0000u : 0u);
}

// the chunk with its dropped elements as +0.0
__device__ __forceinline__ v4i dropout_chunk(v4i v, int64_t e8, const DropArgs& d) {
    u32 m[4];
    dropout_masks(e8, d, m);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (int)((u32)v[c] & m[c]);
    return v;
}

// bit e set: element e of the 8 is kept
__device__ __forceinline__ u32 dropout_keep8(int64_t e8, const DropArgs& d) {
    const uint4 r = dropout_words(e8, d);
    const u32 w[4] = {r.x, r.y, r.z, r.w};
    u32 keep = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) keep |= ((w[c] & 0xffffu) >= d.thr ? 1u << (2 * c) : 0u) | ((w[c] >> 16) >= d.thr ? 2u << (2 * c) : 0u);
    return keep;
}

}  // namespace
