// Quantized attention backward for gfx950: the reference's `sdnq_triton_atten_with_backward` (kernels/triton_atten_backward.py) for the
// default configuration -- int8 Q.K^T (matmul_dtype="int8"), P.V in the value dtype (pv_matmul_dtype=None).
//
//   attn_lse_kernel   <- the save_lse tail of sdnq_attn_kernel (triton_atten.py:328-334): lse = m + log2(l) in the log2-scaled domain, 0 for a
//                        row with no visible key when a mask is given, stored in the output dtype.  A pass of its own over Q.K^T with the
//                        reference's per-block update (triton_atten.py:297-309), so the tuned forward kernels stay as they are.
//   attn_delta_kernel <- get_attn_backward_inputs (triton_atten_backward.py:711-712): delta = sum(out * dO), product rounded in the output
//                        dtype, sum in fp32.
//   attn_bwd_dq_kernel  <- sdnq_attn_bwd_dq_kernel  (triton_atten_backward.py:139-223)
//   attn_bwd_dkv_kernel <- sdnq_attn_bwd_dkv_kernel (triton_atten_backward.py:344-483)
// A backward is three launches: delta, dQ (when asked for), dK / dV (when either is asked for).
//
// Blocks are 32 queries x 32 keys, the block of the forward kernels and of the fixtures.  One wave per workgroup, all matmuls on the
// matrix cores (v_mfma_i32_32x32x32_i8 for Q.K^T, dS.K and Q^T.dS; the bf16 / f16 32x32x16 MFMA for dO.V^T and dO^T.P).
// Operand layouts, the K fragment order and its row permutation pi = attn_kpi: attn_dev.h.  With K as the A operand of Q.K^T, register r of
// lane (g, q) is the score of key 16 (r >> 3) + 8 g + (r & 7) (= sigma(g, r)); with K as the B operand, of query 8 (r >> 2) + 4 g + (r & 3)
// (= tau(g, r)).  A contraction may take its k index in any order common to both operands: the dS tiles feed the next MFMA straight from the
// accumulator registers, and the other operand (K^T, Q^T, dO^T) is staged in LDS in that same order.

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

// ---- dQ: one wave = 32 queries of one head, looping over the key blocks --------------------------------------------------------------
template <int V_T, int D>
__global__ __launch_bounds__(64) void attn_bwd_dq_kernel(const BwdParams p, int64_t qblocks) {
    constexpr int KK = D / 32, KS = D / 16;
    __shared__ __attribute__((aligned(16))) int8_t kt[D * 32];  // K^T of the block: kt[ch][16 g + j] = K[sigma(g, j)][ch]
    const int lane = threadIdx.x, ql = lane & 31, g = lane >> 5;
    const int64_t head_lin = blockIdx.x / qblocks, q0 = (blockIdx.x % qblocks) * 32;
    int64_t z, h, kvh, kvr;
    divmod(head_lin, p.qh, z, h);
    divmod(h * p.kh, p.qh, kvh, kvr);
    const int64_t kv_lin = z * p.kh + kvh;
    const int64_t qi = q0 + ql, qrow = qi < p.qn ? qi : p.qn - 1;
    v4i qf[KK], dof[KS];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[kk] = *(const v4i*)(p.qq + (head_lin * p.qn + qrow) * D + 32 * kk + 16 * g);
    const int64_t go = p.gvst.at(head_lin, qrow);
#pragma unroll
    for (int s = 0; s < KS; ++s) dof[s] = ld_row8(p.gv, go, 16 * s + 8 * g, p.d_src, true);
    const float qsc = p.qs[head_lin * p.qn + qrow];
    const float lse = ld_rt(p.lse, head_lin * p.qn + qrow, p.lse_dtype), delta = p.delta[head_lin * p.qn + qrow];
    const int8_t* kbase = p.kq + kv_lin * p.knp * D;
    const float* ksr = p.ks + kv_lin * p.knp;
    const int kkey = attn_kpi(ql);  // key (inside the block) of this lane's K fragment row / V row
    const int kpos = 16 * ((kkey >> 3) & 1) + 8 * (kkey >> 4) + (kkey & 7);
    v16f acc[KK];
#pragma unroll
    for (int cb = 0; cb < KK; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
    int64_t nkb = p.knp / 32;
    if (p.causal && q0 / 32 + 1 < nkb) nkb = q0 / 32 + 1;  // blocks past the last query are skipped (triton_atten_backward.py:142)
    for (int64_t kb = 0; kb < nkb; ++kb) {
        const int64_t key0 = kb * 32;
        v4i kf[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kf[kk] = *(const v4i*)(kbase + (kb * KK + kk) * 1024 + lane * 16);
        v16i s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf[kk], qf[kk], s, 0, 0, 0);
        // dP^T = V.dO^T (triton_atten_backward.py:183, 195)
        const bool vok = key0 + kkey < p.kn;
        const int64_t vo = p.vst.at(kv_lin, vok ? key0 + kkey : 0);
        v16f dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
#pragma unroll
        for (int st = 0; st < KS; ++st) dp = attn_mfma16<V_T>(ld_row8(p.v, vo, 16 * st + 8 * g, p.d_src, vok), dof[st], dp);
        __syncthreads();  // the previous block's K^T reads are done
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int8_t* b = (const int8_t*)&kf[kk];
#pragma unroll
            for (int j = 0; j < 16; ++j) kt[(32 * kk + 16 * g + j) * 32 + kpos] = b[j];
        }
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t key = key0 + 16 * (r >> 3) + 8 * g + (r & 7);
            const float ksc = ksr[key];
            float qk = (((float)s[r] * qsc) * ksc) * p.log2_sm_scale;  // :161
            qk = attn_bwd_mask(p, qk, z, h, qrow, key);
            const float pr = __builtin_amdgcn_exp2f(qk - lse);          // :180-181
            ds[r] = ((pr * (dp[r] - delta)) * p.sm_scale) * ksc;        // :197-199
        }
        v4i codes;
        const float dss = quant_block(ds, codes);
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < KK; ++cb) {
            const v4i a = *(const v4i*)(kt + (32 * cb + ql) * 32 + 16 * g);
            v16i t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0;
            t = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, codes, t, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = __builtin_fmaf((float)t[r], dss, acc[cb][r]);  // :205
        }
    }
    if (qi >= p.qn) return;
    const int64_t oo = p.dqst.at(head_lin, qi);
#pragma unroll
    for (int cb = 0; cb < KK; ++cb)
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const int c0 = 32 * cb + 8 * t4 + 4 * g;
            if (c0 >= p.dq_ch) continue;
#pragma unroll
            for (int u = 0; u < 4; ++u) st_rt(p.dq, oo + c0 + u, acc[cb][4 * t4 + u], p.grad_dtype);
        }
}

// ---- dK / dV: one wave = 32 keys of one KV head, looping over the query heads of its group and their query blocks -------------------
template <int V_T, int D>
__global__ __launch_bounds__(64) void attn_bwd_dkv_kernel(const BwdParams p, int64_t kblocks) {
    constexpr int KK = D / 32, KS = D / 16;
    __shared__ __attribute__((aligned(16))) int8_t qt[D * 32];      // Q codes^T: qt[ch][16 g + j] = Q[tau(g, j)][ch]
    __shared__ __attribute__((aligned(16))) uint16_t ot[D * 32];    // dO^T: ot[ch][16 c + 8 g + j] = dO[16 c + tau(g, j)][ch], j < 8
    const int lane = threadIdx.x, ql = lane & 31, g = lane >> 5;
    const int64_t kv_lin = blockIdx.x / kblocks, key0 = (blockIdx.x % kblocks) * 32;
    int64_t z, kvh;
    divmod(kv_lin, p.kh, z, kvh);
    const int ratio = (int)(p.qh / p.kh);
    const int kkey = attn_kpi(ql);
    const int64_t key = key0 + kkey;
    const bool kok = key < p.kn;
    const bool want_k = p.dk != nullptr, want_v = p.dv != nullptr;
    v4i kf[KK], vb[KS];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) kf[kk] = *(const v4i*)(p.kq + kv_lin * p.knp * D + ((key0 / 32) * KK + kk) * 1024 + lane * 16);
    const int64_t vo = p.vst.at(kv_lin, kok ? key : 0);
#pragma unroll
    for (int st = 0; st < KS; ++st) vb[st] = ld_row8(p.v, vo, 16 * st + 8 * g, p.d_src, kok);
    const float ksc = p.ks[kv_lin * p.knp + key];
    v16f dk[KK], dv[KK];
#pragma unroll
    for (int cb = 0; cb < KK; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[cb][r] = dv[cb][r] = 0.0f;
    const int64_t nqb = (p.qn + 31) / 32;
    for (int hi = 0; hi < ratio; ++hi) {
        const int64_t h = kvh * ratio + hi, head_lin = z * p.qh + h;
        for (int64_t mb = p.causal ? key0 / 32 : 0; mb < nqb; ++mb) {  // :362-367
            const int64_t q0 = mb * 32;
            const int64_t qrow_a = q0 + ql < p.qn ? q0 + ql : p.qn - 1;  // this lane's row as an A operand
            __syncthreads();  // the previous block's LDS reads are done
            // stage Q codes^T and dO^T of the 32 queries
#pragma unroll
            for (int i = 0; i < D / 32; ++i) {
                const int cid = lane + 64 * i, row = cid / (D / 16), c16 = cid % (D / 16);
                const int64_t q = q0 + row;
                v4i w = (v4i){0, 0, 0, 0};
                if (q < p.qn) w = *(const v4i*)(p.qq + (head_lin * p.qn + q) * D + 16 * c16);
                const int pos = 16 * ((row >> 2) & 1) + 4 * (row >> 3) + (row & 3);
                const int8_t* b = (const int8_t*)&w;
#pragma unroll
                for (int j = 0; j < 16; ++j) qt[(16 * c16 + j) * 32 + pos] = b[j];
            }
            if (want_v) {
#pragma unroll
                for (int i = 0; i < D / 16; ++i) {
                    const int cid = lane + 64 * i, row = cid / (D / 8), c8 = cid % (D / 8);
                    const int64_t q = q0 + row;
                    const v4i w = ld_row8(p.gv, p.gvst.at(head_lin, q < p.qn ? q : 0), 8 * c8, p.d_src, q < p.qn);
                    const int pos = 16 * (row >> 4) + 8 * ((row >> 2) & 1) + 4 * ((row >> 3) & 1) + (row & 3);
                    const uint16_t* e = (const uint16_t*)&w;
#pragma unroll
                    for (int j = 0; j < 8; ++j) ot[(8 * c8 + j) * 32 + pos] = e[j];
                }
            }
            // S = Q.K^T and dP = dO.V^T: lane (g, rho) holds key `key`, register r query q0 + tau(g, r)
            v16i s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0;
            const int8_t* qa = p.qq + (head_lin * p.qn + qrow_a) * D + 16 * g;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const v4i*)(qa + 32 * kk), kf[kk], s, 0, 0, 0);
            v16f dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
            if (want_k) {
                const int64_t go = p.gvst.at(head_lin, qrow_a);
#pragma unroll
                for (int st = 0; st < KS; ++st) dp = attn_mfma16<V_T>(ld_row8(p.gv, go, 16 * st + 8 * g, p.d_src, true), vb[st], dp);
            }
            float pr[16], ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t q = q0 + 8 * (r >> 2) + 4 * g + (r & 3);
                const bool qok = q < p.qn;
                const int64_t qc = qok ? q : p.qn - 1;
                const float qsc = p.qs[head_lin * p.qn + qc];
                float qk = (((float)s[r] * qsc) * ksc) * p.log2_sm_scale;  // :387
                qk = attn_bwd_mask(p, qk, z, h, qc, key);
                const float lse = ld_rt(p.lse, head_lin * p.qn + qc, p.lse_dtype);
                pr[r] = qok ? __builtin_amdgcn_exp2f(qk - lse) : 0.0f;     // :406-408 (rows past the queries contribute nothing)
                ds[r] = ((pr[r] * (dp[r] - p.delta[head_lin * p.qn + qc])) * p.sm_scale) * qsc;  // :428-430
            }
            __syncthreads();  // staged tiles visible
            if (want_k) {
                v4i codes;
                const float dss = quant_block(ds, codes);
#pragma unroll
                for (int cb = 0; cb < KK; ++cb) {
                    const v4i a = *(const v4i*)(qt + (32 * cb + ql) * 32 + 16 * g);
                    v16i t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) t[r] = 0;
                    t = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, codes, t, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) dk[cb][r] = __builtin_fmaf((float)t[r], dss, dk[cb][r]);  // :436
                }
            }
            if (want_v) {  // P in the value dtype, dv += dO^T.P (:473-474)
                v4i pf[2];
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int w = 0; w < 4; ++w) pf[c][w] = (int)pack2<V_T>(pr[8 * c + 2 * w], pr[8 * c + 2 * w + 1]);
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int cb = 0; cb < KK; ++cb) dv[cb] = attn_mfma16<V_T>(*(const v4i*)(ot + (32 * cb + ql) * 32 + 16 * c + 8 * g), pf[c], dv[cb]);
            }
        }
    }
    if (!kok) return;
#pragma unroll
    for (int cb = 0; cb < KK; ++cb)
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const int c0 = 32 * cb + 8 * t4 + 4 * g;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (want_k && c0 < p.dk_ch) st_rt(p.dk, p.dkst.at(kv_lin, key) + c0 + u, dk[cb][4 * t4 + u], p.grad_dtype);
                if (want_v && c0 < p.d_src) st_rt(p.dv, p.dvst.at(kv_lin, key) + c0 + u, dv[cb][4 * t4 + u], p.grad_dtype);
            }
        }
}

int fill_common(BwdParams& p, const void* qq, const float* qs, const void* kq, const float* ks, float sm_scale, int is_causal, const void* mask,
                int mask_dtype, int64_t ms_b, int64_t ms_h, int64_t ms_q, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len,
                int64_t kv_len, int64_t head_dim) {
    if (!qq || !qs || !kq || !ks) return SDNQ_ERR_NULL;
    if (!shape_ok(batch, q_heads, kv_heads, q_len, kv_len, 1)) return SDNQ_ERR_SHAPE;  // (a head dim <= 0 is the next line's)
    if (attn_padded_dim(head_dim) == 0) return SDNQ_ERR_UNSUPPORTED;
    if (!attn_mask_ok(mask, mask_dtype)) return SDNQ_ERR_DTYPE;
    if (((uintptr_t)qq | (uintptr_t)kq) % 16) return SDNQ_ERR_ALIGN;
    p.qq = (const int8_t*)qq; p.qs = qs; p.kq = (const int8_t*)kq; p.ks = ks;
    p.qh = q_heads; p.kh = kv_heads; p.qn = q_len; p.kn = kv_len; p.knp = (kv_len + 31) / 32 * 32;
    p.d_src = (int)head_dim; p.causal = is_causal ? 1 : 0;
    p.sm_scale = sm_scale; p.log2_sm_scale = sm_scale * ATTN_LOG2E;  // triton_atten_backward.py:88
    p.m = {mask, mask_dtype, ms_b, ms_h, ms_q};
    return SDNQ_OK;
}

}  // namespace

extern "C" int sdnq_hip_attn_lse(const void* qq, const float* qs, const void* kq, const float* ks, float sm_scale, int is_causal, const void* mask,
                                 int mask_dtype, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q, void* lse, int lse_dtype,
                                 int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len, int64_t head_dim,
                                 sdnq_stream_t stream) {
    BwdParams p{};
    const int rc = fill_common(p, qq, qs, kq, ks, sm_scale, is_causal, mask, mask_dtype, mask_stride_b, mask_stride_h, mask_stride_q, batch, q_heads,
                               kv_heads, q_len, kv_len, head_dim);
    if (rc != SDNQ_OK) return rc;
    if (!lse) return SDNQ_ERR_NULL;
    if (!float_ok(lse_dtype)) return SDNQ_ERR_DTYPE;
    p.lse = lse; p.lse_dtype = lse_dtype;
    const int64_t qblocks = (q_len + 31) / 32;
    const dim3 grid((unsigned)(batch * q_heads * qblocks)), block(64);
    hipStream_t s = (hipStream_t)stream;
    if (attn_padded_dim(head_dim) == 64) hipLaunchKernelGGL((attn_lse_kernel<64>), grid, block, 0, s, p, qblocks);
    else hipLaunchKernelGGL((attn_lse_kernel<128>), grid, block, 0, s, p, qblocks);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_attn_bwd(const void* qq, const float* qs, const void* kq, const float* ks, const void* v, const int64_t* v_strides, int v_dtype,
                                 const void* out, const int64_t* out_strides, const void* grad, const int64_t* grad_strides, int grad_dtype,
                                 const void* grad_v, const int64_t* grad_v_strides, const void* lse, float sm_scale, int is_causal, const void* mask,
                                 int mask_dtype, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q, float* delta,
                                 void* dq, const int64_t* dq_strides, int64_t dq_channels, void* dk, const int64_t* dk_strides, int64_t dk_channels,
                                 void* dv, const int64_t* dv_strides, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len,
                                 int64_t kv_len, int64_t head_dim, sdnq_stream_t stream) {
    BwdParams p{};
    const int rc = fill_common(p, qq, qs, kq, ks, sm_scale, is_causal, mask, mask_dtype, mask_stride_b, mask_stride_h, mask_stride_q, batch, q_heads,
                               kv_heads, q_len, kv_len, head_dim);
    if (rc != SDNQ_OK) return rc;
    if (!v || !out || !grad || !grad_v || !lse || !delta) return SDNQ_ERR_NULL;
    if (v_dtype != SDNQ_BF16 && v_dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (!float_ok(grad_dtype)) return SDNQ_ERR_DTYPE;
    const int64_t dp = attn_padded_dim(head_dim);
    if ((dq && (dq_channels != head_dim && dq_channels != dp)) || (dk && (dk_channels != head_dim && dk_channels != dp))) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)v | (uintptr_t)grad_v) % 16) return SDNQ_ERR_ALIGN;
    if (!attn_set_strides(v_strides, kv_heads, kv_len, head_dim, p.vst) || !attn_set_strides(grad_v_strides, q_heads, q_len, head_dim, p.gvst)) return SDNQ_ERR_ALIGN;
    attn_set_strides(out_strides, q_heads, q_len, head_dim, p.ost);
    attn_set_strides(grad_strides, q_heads, q_len, head_dim, p.gst);
    attn_set_strides(dq_strides, q_heads, q_len, dq_channels, p.dqst);
    attn_set_strides(dk_strides, kv_heads, kv_len, dk_channels, p.dkst);
    attn_set_strides(dv_strides, kv_heads, kv_len, head_dim, p.dvst);
    p.v = v; p.gv = grad_v; p.out = out; p.g = grad; p.lse = lse; p.lse_dtype = grad_dtype; p.delta = delta; p.grad_dtype = grad_dtype;
    p.dq = dq; p.dq_ch = (int)dq_channels; p.dk = dk; p.dk_ch = (int)dk_channels; p.dv = dv;
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = batch * q_heads * q_len;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, p, rows);
    const int64_t qblocks = (q_len + 31) / 32, kblocks = (kv_len + 31) / 32;
    const dim3 gq((unsigned)(batch * q_heads * qblocks)), gk((unsigned)(batch * kv_heads * kblocks)), block(64);
#define BWD_LAUNCH(VT, DD)                                                                              \
    do {                                                                                                \
        if (dq) hipLaunchKernelGGL((attn_bwd_dq_kernel<VT, DD>), gq, block, 0, s, p, qblocks);          \
        if (dk || dv) hipLaunchKernelGGL((attn_bwd_dkv_kernel<VT, DD>), gk, block, 0, s, p, kblocks);   \
    } while (0)
    if (v_dtype == SDNQ_BF16) { if (dp == 64) BWD_LAUNCH(SDNQ_BF16, 64); else BWD_LAUNCH(SDNQ_BF16, 128); }
    else { if (dp == 64) BWD_LAUNCH(SDNQ_F16, 64); else BWD_LAUNCH(SDNQ_F16, 128); }
#undef BWD_LAUNCH
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
