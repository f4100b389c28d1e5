// What the units that WRITE stored codes share -- quantize.hip (float [N][K] -> codes) and merge.hip (codes + low-rank delta -> codes):
// the probed bit-placement table of the packed formats, the per-element encode step (round / clamp / convert, the reference's
// quant_utils.py:28-56 and packed_float.py:27-82) and the packers.  One definition each, so that the two producers of codes cannot
// disagree.  Moving a site here must leave the kernel's instructions as they were (tools/compare_kernels.py,
// profiles/merge_kernel_compare.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdnq_hip.h"
#include "sdnq_dev.h"
#include "unpack_dev.h"

namespace {

struct PackTable {
    // word bit i (bit i&7 of byte i>>3, or bit i&15 of 16-bit word i>>4) <- bit eb[i] of element el[i] (0xff: unused)
    uint8_t el[240];
    uint8_t eb[240];
    // element a word holds at shift 0 (0xff: none).  The reference ORs those in UNMASKED (packed_int/pack.py, e.g. :115
    // `packed[:, :8] | (packed[:, 8:] << 11)`): a code that does not fit in `bits` bits -- uint9..15 have max = 2^bits in
    // the dtype table and the largest element of every asymmetric group quantizes to exactly that -- leaks its high bits
    // into the word.  Reproduced so that the bytes equal the reference's.
    uint8_t base[16];
    int nbits;
};

struct QuantParams {
    const void* src;
    int64_t ld, N, K;
    int group_size, G;
    int P, SG;  // conv: kernel positions per channel (1 for Linear), scales per output row = G * P
    void* q;
    float* scale;
    float* zp;
    WeightFmt fmt;
    float qmin, qmax;
};

__device__ __forceinline__ uint8_t f32_to_e5m2(float f) {  // RNE, |f| <= 57344 (clamped by the caller)
    u32 u = __float_as_uint(f);
    const u32 sign = (u >> 24) & 0x80u;
    u &= 0x7fffffffu;
    u32 r;
    if (u < 0x38800000u) {  // |f| < 2^-14: subnormal, quantum 2^-16
        r = (u32)__builtin_rintf(__uint_as_float(u) * 65536.0f);
    } else {
        u += 0xfffffu + ((u >> 21) & 1u);
        r = (u >> 21) - (112u << 2);
    }
    return (uint8_t)(sign | r);
}

// f32 (already clamped to the format's range) -> eXmY code; restates packed_float.py:27-73 step by step, including its
// rounding rule (round up only if the top four dropped bits exceed one half) and the exponent re-bias by bit surgery.
__device__ __forceinline__ u32 encode_exmy(float x, int ebits, int mbits, bool is_unsigned) {
    const int drop = 23 - mbits;
    u32 bits = __float_as_uint(x);
    const u32 low = (drop > 4) ? ((1u << (drop - 4)) - 1u) : 0u;
    const u32 top4 = bits & (((1u << drop) - 1u) & ~low);
    if (top4 > (1u << (drop - 1))) bits += (1u << drop);
    const u32 sign = bits >> 31;
    const int bias = (1 << (ebits - 1)) - 1;
    const float min_normal = __uint_as_float((u32)(127 + 1 - bias) << 23);
    const float mag = fabsf(__uint_as_float(bits));
    if (mag < min_normal) {
        // integer mantissa on the 2^(1-bias-M) grid; a carry out of the mantissa lands in exponent bit 0
        const float grid = __uint_as_float((u32)(127 + mbits - 1 + bias) << 23);  // 2^M / min_normal
        bits = ((u32)(int)__builtin_rintf(mag * grid)) << drop;
    }
    const u32 exp8 = (bits >> 23) & 0xffu;
    const u32 mant = (bits >> drop) & ((1u << mbits) - 1u);
    const u32 new_exp = ((exp8 >> 7) << (ebits - 1)) | (exp8 & ((1u << (ebits - 1)) - 1u));
    u32 code = (new_exp << mbits) | mant;
    if (!is_unsigned) code |= sign << (ebits + mbits);
    return code & ((1u << (ebits + mbits + (is_unsigned ? 0 : 1))) - 1u);
}

// The per-element encode step: `code` (u32) from the quotient `q` = w / s or (w - zp) / s (a float lvalue, clobbered): ints round half to
// even and clamp, floats nan_to_num, clamp and convert.  A MACRO, not a function: through a force-inlined function -- by value, by
// reference, returning or storing the code -- quant_pack_kernel came out with other instructions (135 fewer, other registers), and the
// kernels that existed keep their listings (profiles/merge_kernel_compare.txt); the macro leaves the statements at the site as they were.
#define SDNQ_ENCODE_QUOTIENT(code, q, f, is_int, packed, qmin_, qmax_)                                                              \
    do {                                                                                                                            \
        if (is_int) {                                                                                                               \
            /* 0/0 of an all-zero group: round and clamp keep the NaN, the integer cast of the reference turns it into 0 */          \
            const bool is_nan = q != q;                                                                                             \
            q = fminf(fmaxf(__builtin_rintf(q), qmin_), qmax_);                                                                     \
            int iv = is_nan ? 0 : (int)q;                                                                                           \
            if (f.kind == SDNQ_KIND_INT && packed) iv -= (int)qmin_; /* stored as value - min */                                    \
            code = (u32)iv;                                                                                                         \
        } else {                                                                                                                    \
            if (q != q) q = 0.0f; /* nan_to_num_ */                                                                                 \
            else if (q == __builtin_inff()) q = 3.4028234663852886e38f;                                                             \
            else if (q == -__builtin_inff()) q = -3.4028234663852886e38f;                                                           \
            q = fminf(fmaxf(q, qmin_), qmax_);                                                                                      \
            if (f.native_float) {                                                                                                   \
                if (f.bits == 8) code = (f.ebits == 4) ? f32_to_e4m3fn(q) : f32_to_e5m2(q);                                         \
                else code = (f.ebits == 5) ? f32_to_f16_bits(q) : f32_to_bf16_bits(q);                                              \
            } else {                                                                                                                \
                code = encode_exmy(q, f.ebits, f.mbits, f.kind == SDNQ_KIND_UFLOAT);                                                \
            }                                                                                                                       \
        }                                                                                                                           \
    } while (0)

// the 16 codes c[] of elements e0 .. e0 + 15 in the output storage (raw bytes / words, or the reference's group codecs)
__device__ __forceinline__ void store_codes(const QuantParams& p, const PackTable& t, int64_t e0, const u32* c) {
    const WeightFmt f = p.fmt;
    if (f.storage == SDNQ_ST_RAW8) {
        uint8_t* o = (uint8_t*)p.q + e0;
        u32 ww[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) ww[j >> 2] |= (c[j] & 0xffu) << (8 * (j & 3));
        *(uint4*)o = make_uint4(ww[0], ww[1], ww[2], ww[3]);
    } else if (f.storage == SDNQ_ST_RAW16) {
        uint16_t* o = (uint16_t*)p.q + e0;
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = (uint16_t)c[j];
    } else if (f.storage == SDNQ_ST_PACKED_U8) {
        uint8_t* o = (uint8_t*)p.q + (e0 >> 3) * f.bits;
        for (int h = 0; h < 2; ++h) {
            for (int b = 0; b < f.bits; ++b) {
                u32 byte = 0;
                for (int i = 0; i < 8; ++i) {
                    const int wi = b * 8 + i;
                    if (t.el[wi] != 0xff) byte |= ((c[8 * h + t.el[wi]] >> t.eb[wi]) & 1u) << i;
                }
                if (t.base[b] != 0xff) byte |= c[8 * h + t.base[b]] & 0xffu & ~((1u << f.bits) - 1u);
                o[h * f.bits + b] = (uint8_t)byte;
            }
        }
    } else {
        uint16_t* o = (uint16_t*)p.q + (e0 >> 4) * f.bits;
        for (int b = 0; b < f.bits; ++b) {
            u32 word = 0;
            for (int i = 0; i < 16; ++i) {
                const int wi = b * 16 + i;
                if (t.el[wi] != 0xff) word |= ((c[t.el[wi]] >> t.eb[wi]) & 1u) << i;
            }
            if (t.base[b] != 0xff) word |= c[t.base[b]] & 0xffffu & ~((1u << f.bits) - 1u);
            o[b] = (uint16_t)word;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the table of a packed storage, probed from the decoders of unpack_dev.h one word bit at a time (raw storages: an empty table)
int build_table(int storage, int bits, PackTable& t) {
    for (int i = 0; i < 240; ++i) { t.el[i] = 0xff; t.eb[i] = 0; }
    t.nbits = 0;
    if (storage == SDNQ_ST_PACKED_U8) {
        t.nbits = 8 * bits;
        for (int i = 0; i < t.nbits; ++i) {
            uint8_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            w[i >> 3] = (uint8_t)(1u << (i & 7));
            u32 e[8];
            unpack8_u8(w, bits, e);
            for (int j = 0; j < 8; ++j) {
                const u32 v = e[j] & ((1u << bits) - 1u);
                if (v) { t.el[i] = (uint8_t)j; t.eb[i] = (uint8_t)__builtin_ctz(v); break; }
            }
        }
    } else if (storage == SDNQ_ST_PACKED_I16) {
        t.nbits = 16 * bits;
        for (int i = 0; i < t.nbits; ++i) {
            uint16_t w[16] = {0};
            w[i >> 4] = (uint16_t)(1u << (i & 15));
            u32 e[16];
            unpack16_i16(w, bits, e);
            for (int j = 0; j < 16; ++j) {
                const u32 v = e[j] & ((1u << bits) - 1u);
                if (v) { t.el[i] = (uint8_t)j; t.eb[i] = (uint8_t)__builtin_ctz(v); break; }
            }
        }
    }
    const int wbits = (storage == SDNQ_ST_PACKED_U8) ? 8 : 16;
    for (int w = 0; w < 16; ++w) t.base[w] = 0xff;
    for (int w = 0; w < bits && t.nbits; ++w) {
        const int e = t.el[w * wbits];
        bool is_base = e != 0xff;
        for (int b = 0; b < bits && is_base; ++b) is_base = (t.el[w * wbits + b] == e && t.eb[w * wbits + b] == b);
        if (is_base) t.base[w] = (uint8_t)e;
    }
    // every element bit must be fed by exactly one word bit
    if (t.nbits) {
        int seen[16] = {0};
        for (int i = 0; i < t.nbits; ++i)
            if (t.el[i] != 0xff) seen[t.el[i]] |= 1 << t.eb[i];
        const int elems = (storage == SDNQ_ST_PACKED_U8) ? 8 : 16;
        for (int j = 0; j < elems; ++j)
            if (seen[j] != (1 << bits) - 1) return SDNQ_ERR_UNSUPPORTED;
    }
    return SDNQ_OK;
}

}  // namespace
