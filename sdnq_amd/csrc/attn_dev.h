// What the attention units share -- attention.hip (the tuned default forward and its prepare pass), attention_var.hip (the other matmul
// formats) and attention_bwd.hip (lse, delta, dQ, dK / dV): strides, the operand layouts, the per-token quantization pieces, the small
// wave idioms and the checks of the entry points.  One definition each.  Everything sits in an anonymous namespace, as the kernels do:
// their mangled names (the keys of tools/compare_kernels.py and of profiles/*kernel_stats*) name these types.
// Folding a site into a helper must leave the kernel's instructions as they were: tools/compare_kernels.py shows it.  Where it did not,
// the site keeps its own spelling (profiles/attn_dev_kernel_compare.txt): the token-row ingest of the two prepare kernels, the mask /
// causal / key-tail arithmetic of attn_fwd_var_kernel and of the backward kernels, attn_fwd_var_kernel's block maximum and its P.V in the value dtype.
//
// Operand layouts (lane l = 32 g + i of a wave; kk = 32-channel step, D = head dim padded to 64 / 128):
//   32x32x32 i8:     A row i, bytes k = 16 g .. 16 g + 15;  B column i, the same k
//   32x32x16 16-bit: A row i, elements k = 8 g .. 8 g + 7;  B column i, the same k
//   result:          column i, register r <-> row 8 (r >> 2) + 4 g + (r & 3)
//   K codes (int8 and e4m3 bytes alike): one 1-KiB tile per (32-key block, kk); lane (g, rho) holds the 16 bytes [32 kk + 16 g, +16) of key
//   pi(rho), pi = attn_kpi = swap bits 2 and 3 of the row index.  With K as the A operand of S^T = K.Q^T, registers 8c .. 8c + 7 of lane
//   (g, query) are then the CONTIGUOUS keys 16 c + 8 g .. + 7, register r <-> key 16 (r >> 3) + 8 g + (r & 7): exactly the K-slice that
//   lane feeds to P.V MFMA c, so P never moves between lanes, and every fragment load is one fully coalesced 16-bytes-per-lane access.
//   V in the value dtype (attn_vt_block): one 1-KiB tile per (32-key block kb, 32-channel block dd, 16-key step c); lane (g, ql) holds the
//   8 keys 32 kb + 16 c + 8 g + 0..7 of channel 32 dd + ql: the first operand of P.V MFMA (dd, c).
#pragma once
#include "hadamard_dev.h"
#include "sdnq_dev.h"

typedef float v2f __attribute__((ext_vector_type(2)));

// crosses the attention units (internal to the library, C++ linkage): attention.hip's launch of attn_var_kmean_kernel -- kmean[batch * kv_heads][d]
// = the channel means of K; arguments already validated by the caller (sdnq_hip_attn_prepare_ex)
void sdnq_internal_attn_kmean(const void* k, const int64_t* k_strides, int dtype, int64_t batch, int64_t kv_heads, int64_t kv_len, int64_t head_dim,
                              float* kmean, hipStream_t s);

namespace {

// element strides of a [batch][heads][tokens][head_dim] tensor whose head_dim is contiguous (e.g. the transposed view of a
// [batch][tokens][heads * head_dim] projection output); `heads` splits a linear batch*heads index
struct Strides {
    int64_t b, h, n, heads;
    __device__ __forceinline__ int64_t at(int64_t head_lin, int64_t tok) const {
        int64_t zb, hh;
        divmod(head_lin, heads, zb, hh);
        return zb * b + hh * h + tok * n;
    }
};

// attention mask [*, *, q, key] (key stride 1) or nullptr.  mask_dtype -1: int8 / bool (0 = masked out), else SdnqFloat of an additive mask;
// element strides, 0 for broadcast dimensions
struct AttnMask {
    const void* mask;
    int mask_dtype;
    int64_t ms_z, ms_h, ms_q;
};

__device__ __forceinline__ int attn_kpi(int rho) { return (rho & 0x13) | ((rho & 4) << 1) | ((rho & 8) >> 1); }

// byte offset of the 8 codes (key n, channels [c8, c8 + 8)) inside one head's K operand (layout above)
__device__ __forceinline__ int64_t attn_kfrag_offset(int64_t n, int c8, int d) {
    const int kk = c8 >> 5, g = (c8 >> 4) & 1, half = (c8 >> 3) & 1, rho = attn_kpi((int)(n & 31));
    return ((n / 32) * (d / 32) + kk) * 1024 + (g * 32 + rho) * 16 + half * 8;
}

// max with lane ^ 32, where the other 16 scores of a row / column live: one v_permlane32_swap (VALU) instead of a trip through LDS
__device__ __forceinline__ float attn_max32(float m) {
    const u32 mb = __float_as_uint(m);
    const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// the 32x32x16 MFMA of the value dtype
template <int V_T>
__device__ __forceinline__ v16f attn_mfma16(v4i a, v4i b, v16f c) {
    if constexpr (V_T == SDNQ_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

// ---- channel means of ONE head's K by one 256-thread workgroup (short key sequences: no separate channel-sum section) --------
// Thread tid owns channels [8 (tid % lpr), + 8) of the rows tid / lpr, + 256 / lpr, ...: `acc` = its sums in row order.  xw: 4 * 128 floats,
// smean: 128 floats of LDS.  One summation order for every caller (the prepare kernels and the single-launch attention), so every route
// produces the same K codes.
__device__ __forceinline__ void attn_means_reduce(float (&acc)[8], int64_t kn, int d, float* xw, float* smean) {
    const int lpr = d / 8, tid = threadIdx.x, c8 = (tid & (lpr - 1)) * 8;  // d is 64 or 128
    // the lanes of a wave that hold the same channels are lpr apart (lane exchange on the VALU / swizzle paths, hadamard_dev.h)
    if (lpr == 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += lane_xor(acc[e], 8);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += lane_xor(acc[e], 16);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += lane_xor(acc[e], 32);
    if ((tid & 63) < lpr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) xw[(tid >> 6) * 128 + c8 + e] = acc[e];
    }
    __syncthreads();
    if (tid < d) smean[tid] = ((xw[tid] + xw[128 + tid]) + (xw[256 + tid] + xw[384 + tid])) / (float)kn;  // k.mean(dim=2), triton_atten.py:459
    __syncthreads();
}
template <int T_ID>
__device__ __forceinline__ void attn_head_means(const void* __restrict__ k, const Strides kst, int64_t head, int64_t kn, int d, int d_src, float* xw, float* smean) {
    const int lpr = d / 8, lsh = d == 64 ? 3 : 4, rpp = 256 >> lsh, tid = threadIdx.x, c8 = (tid & (lpr - 1)) * 8;  // d is 64 or 128
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint16_t* khead = (const uint16_t*)k + kst.at(head, 0);
    for (int64_t r = tid >> lsh; r < kn; r += rpp) {
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (c8 < d_src) Vec16<T_ID>::unpack(*(const uint4*)(khead + r * kst.n + c8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
    attn_means_reduce(acc, kn, d, xw, smean);
}

// ---- one token row spread over lpr = d / 8 lanes, 8 channels each ---------------------------------------------------------------------
// max |v| over the row
__device__ __forceinline__ float attn_row_amax(const float (&v)[8], int lpr) {
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
    amax = fmaxf(amax, lane_xor(amax, 1));
    amax = fmaxf(amax, lane_xor(amax, 2));
    amax = fmaxf(amax, lane_xor(amax, 4));
    if (lpr == 16) amax = fmaxf(amax, lane_xor(amax, 8));
    return amax;
}
// per-token symmetric int8: codes of this lane's 8 channels, the row's scale
__device__ __forceinline__ float attn_quant8(const float (&v)[8], int lpr, u32 (&o)[2]) {
    const float scale = attn_row_amax(v, lpr) / 127.0f;
    RowDiv rd;  // the correctly rounded 3-instruction division (sdnq_dev.h) when every row of the wave has an ordinary scale
    rd.set(scale);
    if (__all(rd.fast)) {
#pragma unroll
        for (int w = 0; w < 2; ++w)
            o[w] = pack4_rne_i8(fastdiv2((pv2f){v[4 * w], v[4 * w + 1]}, rd), fastdiv2((pv2f){v[4 * w + 2], v[4 * w + 3]}, rd));
        return scale;
    }
    // a zero row (scale 0: 0 / 0 must become code 0), a non-finite one or an extreme scale somewhere in the wave: the plain sequence
    o[0] = o[1] = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float q = __builtin_rintf(v[e] / scale);
        if (q != q) q = 0.0f;
        q = fminf(fmaxf(q, -128.0f), 127.0f);
        o[e >> 2] |= ((u32)(int)q & 0xffu) << (8 * (e & 3));
    }
    return scale;
}

// ---- V [heads][kn][d] -> P.V operand in MFMA-fragment order (layout above; knp = kn rounded up to 32, zero padded) ---------------------
template <int PITCH>
__device__ __forceinline__ void attn_vt_block(const uint16_t* __restrict__ v, const Strides vst, uint16_t* __restrict__ vt, int64_t kn, int64_t knp, int d,
                                              int64_t head, int64_t kb, uint16_t (*tile)[PITCH], int d_src) {
    const int64_t key0 = kb * 32;
    const int lpr = d / 8, kkn = d / 32;
    uint16_t* dst = vt + (head * (knp / 32) + kb) * (int64_t)(kkn * 2 * 512);
    const int lsh = d == 64 ? 3 : 4;  // d is 64 or 128
    const uint16_t* vhead = v + vst.at(head, 0);
    for (int t = threadIdx.x; t < 32 * lpr; t += 256) {
        const int kr = t >> lsh, c8 = (t & (lpr - 1)) * 8;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (key0 + kr < kn && c8 < d_src) val = *(const uint4*)(vhead + (key0 + kr) * vst.n + c8);
        const uint16_t* h = (const uint16_t*)&val;
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[kr][c8 + e] = h[e];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kkn * 2 * 64; t += 256) {
        const int lane = t & 63, c = (t >> 6) & 1, dd = t >> 7;
        const int dch = 32 * dd + (lane & 31), k8 = 16 * c + 8 * (lane >> 5);
        u32 w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (u32)tile[k8 + 2 * e][dch] | ((u32)tile[k8 + 2 * e + 1][dch] << 16);
        *(uint4*)(dst + (int64_t)t * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---- host side: the checks every entry point makes, in one spelling ---------------------------------------------------------------------
constexpr float ATTN_LOG2E = 1.4426950408889634f;  // scores live in the log2 domain: log2_sm_scale = sm_scale * log2(e), triton_atten.py:203

inline bool shape_ok(int64_t batch, int64_t qh, int64_t kh, int64_t qn, int64_t kn, int64_t d) {
    return batch > 0 && qh > 0 && kh > 0 && qn > 0 && kn > 0 && d > 0 && qh % kh == 0;
}
inline bool float_ok(int dt) { return dt == SDNQ_F32 || dt == SDNQ_BF16 || dt == SDNQ_F16; }
inline bool attn_mask_ok(const void* mask, int mask_dtype) { return !mask || mask_dtype == -1 || float_ok(mask_dtype); }
// the kernels' head dim: 64 or 128, the extra channels are zeros (0: a head dim that is not built)
inline int64_t attn_padded_dim(int64_t head_dim) { return (head_dim < 8 || head_dim > 128 || head_dim % 8) ? 0 : (head_dim <= 64 ? 64 : 128); }
// log2 of the Hadamard group (0 = no rotation), -1 for a group the padded head dim `d` cannot take
inline int attn_log2g(int group, int64_t d) {
    if (group == 0) return 0;
    if (group < 4 || group > d || (group & (group - 1)) || d % group) return -1;
    int log2g = 0;
    while ((1 << log2g) < group) ++log2g;
    return log2g;
}
// strides from the caller or those of a contiguous [batch][heads][len][ch]; false unless every stride is a multiple of `align` elements
// (8: 16-byte rows of 16-bit elements)
inline bool attn_set_strides(const int64_t* st, int64_t heads, int64_t len, int64_t ch, Strides& o, int align = 8) {
    o.heads = heads;
    if (st) { o.b = st[0]; o.h = st[1]; o.n = st[2]; } else { o.b = heads * len * ch; o.h = len * ch; o.n = ch; }
    return o.b % align == 0 && o.h % align == 0 && o.n % align == 0;
}

}  // namespace
