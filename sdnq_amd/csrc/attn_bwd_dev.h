// What the two backward units share -- attention_bwd.hip (head dims up to 128) and attention_wide_bwd.hip (136 .. 256): the kernel
// parameters, the mask / causal / key-tail arithmetic of one score, the row loads, the per-(row, 32-block) int8 quantizer of dS, and the two
// kernels that are generic in the head dim as they stand: attn_lse_kernel<D> and attn_delta_kernel.  Anonymous namespace as attn_dev.h: the
// kernels' mangled names stay what they were.
#pragma once
#include "attn_dev.h"

namespace {

struct BwdParams {
    const int8_t* qq; const float* qs; const int8_t* kq; const float* ks;
    const void* v; Strides vst;               // value dtype, d_src channels
    const void* gv; Strides gvst;             // dO in the value dtype (the matmul operand)
    const void* out; Strides ost;             // out and dO in the grad dtype (delta)
    const void* g; Strides gst;
    const void* lse; int lse_dtype;
    float* delta;
    AttnMask m;
    void* dq; Strides dqst; int dq_ch;
    void* dk; Strides dkst; int dk_ch;
    void* dv; Strides dvst;
    int grad_dtype;
    int64_t qh, kh, qn, kn, knp;
    int d_src, causal;
    float sm_scale, log2_sm_scale;
};

// mask / causal / key tail of one score (triton_atten_backward.py:170-178)
__device__ __forceinline__ float attn_bwd_mask(const BwdParams& p, float qk, int64_t z, int64_t h, int64_t q, int64_t key) {
    if (p.causal && key > q) return -__builtin_inff();
    if (key >= p.kn) return -__builtin_inff();
    if (p.m.mask != nullptr) {
        const int64_t i = z * p.m.ms_z + h * p.m.ms_h + q * p.m.ms_q + key;
        if (p.m.mask_dtype == -1) return ((const int8_t*)p.m.mask)[i] != 0 ? qk : -__builtin_inff();
        return qk + ld_rt(p.m.mask, i, p.m.mask_dtype);
    }
    return qk;
}

// 8 elements [c0, c0 + 8) of a row in the value dtype, zero past the row's channels
__device__ __forceinline__ v4i ld_row8(const void* base, int64_t off, int c0, int d_src, bool ok) {
    if (!ok || c0 >= d_src) return (v4i){0, 0, 0, 0};
    return *(const v4i*)((const uint16_t*)base + off + c0);
}

// per-(row, block) int8 of 16 values of this lane + 16 of lane ^ 32 (triton_atten_backward.py:200-204 / 431-435): s = max|x| / 127
// (1 where <= 2e-38), code = floor(fma(x, 1 / s, 0.5)); returns s, the codes as the k = 16 bytes of an i8 MFMA operand (byte j = x[j])
__device__ __forceinline__ float quant_block(const float (&x)[16], v4i& codes) {
    float mx = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, __builtin_fabsf(x[r]));
    mx = attn_max32(mx);
    float s = mx * (float)(1.0 / 127.0);
    if (s <= 2e-38f) s = 1.0f;
    const float inv = 1.0f / s;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        u32 word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) word |= ((u32)(int)__builtin_floorf(__builtin_fmaf(x[4 * w + e], inv, 0.5f)) & 0xffu) << (8 * e);
        codes[w] = (int)word;
    }
    return s;
}

// ---- lse: one wave = 32 queries, the reference forward's online max / sum ----------------------------------------------------------
template <int D>
__global__ __launch_bounds__(64) void attn_lse_kernel(const BwdParams p, int64_t qblocks) {
    constexpr int KK = D / 32;
    const int lane = threadIdx.x, ql = lane & 31, g = lane >> 5;
    const int64_t head_lin = blockIdx.x / qblocks, q0 = (blockIdx.x % qblocks) * 32;
    int64_t z, h, kvh, kvr;
    divmod(head_lin, p.qh, z, h);
    divmod(h * p.kh, p.qh, kvh, kvr);
    const int64_t kv_lin = z * p.kh + kvh;
    const int64_t qi = q0 + ql, qrow = qi < p.qn ? qi : p.qn - 1;
    v4i qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[kk] = *(const v4i*)(p.qq + (head_lin * p.qn + qrow) * D + 32 * kk + 16 * g);
    const float qsc = p.qs[head_lin * p.qn + qrow];
    const int8_t* kbase = p.kq + kv_lin * p.knp * D;
    const float* ksr = p.ks + kv_lin * p.knp;
    int64_t nkb = p.knp / 32;
    if (p.causal && q0 / 32 + 1 < nkb) nkb = q0 / 32 + 1;
    float m_i = -__builtin_inff(), l_i = 0.0f;
    for (int64_t kb = 0; kb < nkb; ++kb) {
        v16i s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const v4i*)(kbase + (kb * KK + kk) * 1024 + lane * 16), qf[kk], s, 0, 0, 0);
        float t[16];
        float mb = -__builtin_inff();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t key = kb * 32 + 16 * (r >> 3) + 8 * g + (r & 7);
            const float qk = (((float)s[r] * qsc) * ksr[key]) * p.log2_sm_scale;  // triton_atten.py:278
            t[r] = attn_bwd_mask(p, qk, z, h, qrow, key);
            mb = fmaxf(mb, t[r]);
        }
        const float m_ij = fmaxf(m_i, attn_max32(mb));
        float alpha, sub;
        if (p.m.mask != nullptr) {  // triton_atten.py:299-301
            alpha = __builtin_amdgcn_exp2f((m_i == -__builtin_inff() && m_ij == -__builtin_inff()) ? 0.0f : m_i - m_ij);
            sub = m_ij == -__builtin_inff() ? 0.0f : m_ij;
        } else {
            alpha = __builtin_amdgcn_exp2f(m_i - m_ij);
            sub = m_ij;
        }
        float ps = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ps += __builtin_amdgcn_exp2f(t[r] - sub);
        ps += __shfl_xor(ps, 32);
        l_i = __builtin_fmaf(l_i, alpha, ps);
        m_i = m_ij;
    }
    if (qi >= p.qn || g != 0) return;
    float lse = m_i + __builtin_log2f(l_i);  // :329
    if (p.m.mask != nullptr && lse == -__builtin_inff()) lse = 0.0f;
    st_rt((void*)p.lse, head_lin * p.qn + qi, lse, p.lse_dtype);
}

// ---- delta = sum(out * dO): one thread per query row ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_delta_kernel(const BwdParams p, int64_t rows) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int64_t head_lin = row / p.qn, q = row % p.qn;
    const int64_t oo = p.ost.at(head_lin, q), go = p.gst.at(head_lin, q);
    float acc = 0.0f;
    for (int c = 0; c < p.d_src; ++c)
        acc += round_rt(ld_rt(p.out, oo + c, p.grad_dtype) * ld_rt(p.g, go + c, p.grad_dtype), p.grad_dtype);
    p.delta[row] = acc;
}

}  // namespace
