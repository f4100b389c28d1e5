// Quantized attention backward for head dims 136 .. 256 on gfx950: attention_bwd.hip's arithmetic (the reference's
// sdnq_triton_atten_bwd, kernels/triton_atten_backward.py:728-841, for int8 Q.K^T and P.V in the value dtype) where that unit stops at 128.
// The head dim is padded to DP in {160, 192, 224, 256} as the forward pads it (attention_wide.hip); the operands are the Q / K codes and
// scales that sdnq_hip_attn_wide's prepare pass left in its workspace.
//
//   attn_lse_kernel<DP>, attn_delta_kernel  <- attn_bwd_dev.h, as they stand
//   attn_wide_bwd_dq_kernel                 <- sdnq_attn_bwd_dq_kernel  (triton_atten_backward.py:139-223)
//   attn_wide_bwd_dkv_kernel                <- sdnq_attn_bwd_dkv_kernel (triton_atten_backward.py:344-483)
//
// Why another work split.  attention_bwd.hip's wave keeps every accumulator of its 32 rows: dk[D / 32] and dv[D / 32] in the dK / dV kernel
// (256 registers at D = 256 before any operand), dq[D / 32] next to the Q and dO fragments in the dQ kernel (128 + 32 + 64).  Here
//   dK / dV: a workgroup of TWO waves owns 32 keys of one KV head and the waves split the OUTPUTS: wave 0 computes S, dP and dS, quantizes dS
//            and accumulates dK; wave 1 computes S and P and accumulates dV.  Each holds DP / 32 accumulator tiles (128 registers at most) in
//            ONE array, whichever role it has.  The K fragment tiles and the V fragments of the 32 keys, which the narrow kernel keeps in
//            registers (32 + 64 at DP = 256), sit in LDS, loaded once; the Q^T code tile (wave 0's operand) and the dO^T tile (wave 1's) of
//            the current 32 queries are staged in LDS by all 128 threads.  With only one of dK / dV wanted the other wave stages and idles.
//   dQ:      a PAIR of waves owns 32 queries and splits the CHANNEL TILES of dQ, as the forward does with O: both compute S, dP, dS and its
//            codes (the same operands in the same order, so the same bits); each transposes the K tiles of its own channels into LDS and
//            accumulates ceil / floor of DP / 64 tiles (64 registers at most).  The price is the score arithmetic twice; splitting the dP
//            contraction instead would change the order of a floating-point sum.
// Every floating-point sum keeps the narrow kernels' order (channel steps ascending inside dP, key / query blocks ascending, the query heads
// of a group in order, one fmaf per block for dQ / dK), so on operands that are zero above channel 128 the results equal attention_bwd.hip's
// bit for bit.  No atomics; the same bits on every call.
#include "attn_bwd_dev.h"
#include "attn_wide_dev.h"

namespace {

// ---- dQ: a pair of waves = 32 queries of one head; wave `half` owns the channel tiles [half * NT, ...) -----------------------------------
template <int V_T, int DP>
__global__ __launch_bounds__(128) void attn_wide_bwd_dq_kernel(const BwdParams p, int64_t qblocks) {
    constexpr int KK = DP / 32, KS = DP / 16;
    constexpr int NT = (KK + 1) / 2;  // channel tiles of the first wave; the second has KK - NT (one fewer when KK is odd)
    __shared__ __attribute__((aligned(16))) int8_t kt[DP * 32];  // K^T of the block: kt[ch][16 g + j] = K[sigma(g, j)][ch]; rows written and read by the wave that owns ch
    const int lane = threadIdx.x & 63, half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ql = lane & 31, g = lane >> 5;
    const int t0 = half * NT, nt = half == 0 ? NT : KK - NT;  // wave-uniform
    const int64_t head_lin = blockIdx.x / qblocks, q0 = (blockIdx.x % qblocks) * 32;
    int64_t z, h, kvh, kvr;
    divmod(head_lin, p.qh, z, h);
    divmod(h * p.kh, p.qh, kvh, kvr);
    const int64_t kv_lin = z * p.kh + kvh;
    const int64_t qi = q0 + ql, qrow = qi < p.qn ? qi : p.qn - 1;
    v4i qf[KK], dof[KS];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[kk] = *(const v4i*)(p.qq + (head_lin * p.qn + qrow) * DP + 32 * kk + 16 * g);
    const int64_t go = p.gvst.at(head_lin, qrow);
#pragma unroll
    for (int s = 0; s < KS; ++s) dof[s] = ld_row8(p.gv, go, 16 * s + 8 * g, p.d_src, true);
    const float qsc = p.qs[head_lin * p.qn + qrow];
    const float lse = ld_rt(p.lse, head_lin * p.qn + qrow, p.lse_dtype), delta = p.delta[head_lin * p.qn + qrow];
    const int8_t* kbase = p.kq + kv_lin * p.knp * DP;
    const float* ksr = p.ks + kv_lin * p.knp;
    const int kkey = attn_kpi(ql);  // key (inside the block) of this lane's K fragment row / V row
    const int kpos = 16 * ((kkey >> 3) & 1) + 8 * (kkey >> 4) + (kkey & 7);
    v16f acc[NT];
#pragma unroll
    for (int dd = 0; dd < NT; ++dd)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dd][r] = 0.0f;
    int64_t nkb = p.knp / 32;
    if (p.causal && q0 / 32 + 1 < nkb) nkb = q0 / 32 + 1;  // blocks past the last query are skipped (triton_atten_backward.py:142)
    for (int64_t kb = 0; kb < nkb; ++kb) {  // the same trip count in both waves: the barriers below are workgroup-uniform
        const int64_t key0 = kb * 32;
        v4i kf[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kf[kk] = *(const v4i*)(kbase + (kb * KK + kk) * 1024 + lane * 16);
        v16i s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf[kk], qf[kk], s, 0, 0, 0);
        __syncthreads();  // the previous block's K^T reads are done
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
            if (kk / NT == half) {  // this wave's channel tiles
                const int8_t* b = (const int8_t*)&kf[kk];
#pragma unroll
                for (int j = 0; j < 16; ++j) kt[(32 * kk + 16 * g + j) * 32 + kpos] = b[j];
            }
        // dP^T = V.dO^T (triton_atten_backward.py:183, 195), channel steps ascending
        const bool vok = key0 + kkey < p.kn;
        const int64_t vo = p.vst.at(kv_lin, vok ? key0 + kkey : 0);
        v16f dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
#pragma unroll
        for (int st = 0; st < KS; ++st) dp = attn_mfma16<V_T>(ld_row8(p.v, vo, 16 * st + 8 * g, p.d_src, vok), dof[st], dp);
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
        for (int dd = 0; dd < NT; ++dd)
            if (dd < nt) {
                const v4i a = *(const v4i*)(kt + (32 * (t0 + dd) + ql) * 32 + 16 * g);
                v16i t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0;
                t = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, codes, t, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[dd][r] = __builtin_fmaf((float)t[r], dss, acc[dd][r]);  // :205
            }
    }
    if (qi >= p.qn) return;
    const int64_t oo = p.dqst.at(head_lin, qi);
#pragma unroll
    for (int dd = 0; dd < NT; ++dd)
        if (dd < nt) {
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int c0 = 32 * (t0 + dd) + 8 * t4 + 4 * g;
                if (c0 >= p.dq_ch) continue;
#pragma unroll
                for (int u = 0; u < 4; ++u) st_rt(p.dq, oo + c0 + u, acc[dd][4 * t4 + u], p.grad_dtype);
            }
        }
}

// ---- dK / dV: two waves = 32 keys of one KV head, looping over the query heads of the group and their query blocks; wave 0 accumulates dK,
// ---- wave 1 dV, in the one array `acc` -------------------------------------------------------------------------------------------------------
template <int V_T, int DP>
__global__ __launch_bounds__(128) void attn_wide_bwd_dkv_kernel(const BwdParams p, int64_t kblocks) {
    constexpr int KK = DP / 32, KS = DP / 16;
    __shared__ __attribute__((aligned(16))) int8_t qt[DP * 32];        // Q codes^T: qt[ch][16 g + j] = Q[tau(g, j)][ch]            (wave 0 reads)
    __shared__ __attribute__((aligned(16))) uint16_t ot[DP * 32];      // dO^T: ot[ch][16 c + 8 g + j] = dO[16 c + tau(g, j)][ch]   (wave 1 reads)
    __shared__ __attribute__((aligned(16))) int8_t kl[KK * 1024];      // the K fragment tiles of the 32 keys, as in memory        (both read)
    __shared__ __attribute__((aligned(16))) uint16_t vl[KS * 64 * 8];  // V fragments: vl[st][lane] = V[key of lane][16 st + 8 g, + 8) (wave 0 reads)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, g = lane >> 5;
    const int64_t kv_lin = blockIdx.x / kblocks, key0 = (blockIdx.x % kblocks) * 32;
    int64_t z, kvh;
    divmod(kv_lin, p.kh, z, kvh);
    const int ratio = (int)(p.qh / p.kh);
    const int kkey = attn_kpi(ql);
    const int64_t key = key0 + kkey;
    const bool kok = key < p.kn;
    const bool want_k = p.dk != nullptr, want_v = p.dv != nullptr;
    const bool mine = wave == 0 ? want_k : want_v;  // wave-uniform: this wave has an output to accumulate
    {
        const v4i* ksrc = (const v4i*)(p.kq + kv_lin * p.knp * DP + (key0 / 32) * (KK * 1024));
        for (int i = tid; i < KK * 64; i += 128) ((v4i*)kl)[i] = ksrc[i];
        if (want_k) {
            for (int i = tid; i < KS * 64; i += 128) {
                const int st = i >> 6, l = i & 63;
                const int64_t vkey = key0 + attn_kpi(l & 31);
                const bool ok = vkey < p.kn;
                ((v4i*)vl)[i] = ld_row8(p.v, p.vst.at(kv_lin, ok ? vkey : 0), 16 * st + 8 * (l >> 5), p.d_src, ok);
            }
        }
    }
    const float ksc = p.ks[kv_lin * p.knp + key];
    v16f acc[KK];
#pragma unroll
    for (int cb = 0; cb < KK; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
    const int64_t nqb = (p.qn + 31) / 32;
    for (int hi = 0; hi < ratio; ++hi) {
        const int64_t h = kvh * ratio + hi, head_lin = z * p.qh + h;
        for (int64_t mb = p.causal ? key0 / 32 : 0; mb < nqb; ++mb) {  // :362-367
            const int64_t q0 = mb * 32;
            const int64_t qrow_a = q0 + ql < p.qn ? q0 + ql : p.qn - 1;  // this lane's row as an A operand
            __syncthreads();  // the previous block's LDS reads are done (first trip: the K / V tiles are written)
            // stage Q codes^T and dO^T of the 32 queries, all 128 threads
            if (want_k) {
                for (int cid = tid; cid < 2 * DP; cid += 128) {
                    const int row = cid / (DP / 16), c16 = cid % (DP / 16);
                    const int64_t q = q0 + row;
                    v4i w = (v4i){0, 0, 0, 0};
                    if (q < p.qn) w = *(const v4i*)(p.qq + (head_lin * p.qn + q) * DP + 16 * c16);
                    const int pos = 16 * ((row >> 2) & 1) + 4 * (row >> 3) + (row & 3);
                    const int8_t* b = (const int8_t*)&w;
#pragma unroll
                    for (int j = 0; j < 16; ++j) qt[(16 * c16 + j) * 32 + pos] = b[j];
                }
            }
            if (want_v) {
                for (int cid = tid; cid < 4 * DP; cid += 128) {
                    const int row = cid / (DP / 8), c8 = cid % (DP / 8);
                    const int64_t q = q0 + row;
                    const v4i w = ld_row8(p.gv, p.gvst.at(head_lin, q < p.qn ? q : 0), 8 * c8, p.d_src, q < p.qn);
                    const int pos = 16 * (row >> 4) + 8 * ((row >> 2) & 1) + 4 * ((row >> 3) & 1) + (row & 3);
                    const uint16_t* e = (const uint16_t*)&w;
#pragma unroll
                    for (int j = 0; j < 8; ++j) ot[(8 * c8 + j) * 32 + pos] = e[j];
                }
            }
            // S = Q.K^T (both roles) and dP = dO.V^T (wave 0): lane (g, rho) holds key `key`, register r query q0 + tau(g, r)
            float pr[16], ds[16];
            if (mine) {
                v16i s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0;
                const int8_t* qa = p.qq + (head_lin * p.qn + qrow_a) * DP + 16 * g;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk)
                    s = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const v4i*)(qa + 32 * kk), *(const v4i*)(kl + kk * 1024 + lane * 16), s, 0, 0, 0);
                v16f dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
                if (wave == 0) {
                    const int64_t go = p.gvst.at(head_lin, qrow_a);
#pragma unroll
                    for (int st = 0; st < KS; ++st)
                        dp = attn_mfma16<V_T>(ld_row8(p.gv, go, 16 * st + 8 * g, p.d_src, true), *(const v4i*)(vl + (st * 64 + lane) * 8), dp);
                }
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
                    ds[r] = 0.0f;
                    if (wave == 0) ds[r] = ((pr[r] * (dp[r] - p.delta[head_lin * p.qn + qc])) * p.sm_scale) * qsc;  // :428-430
                }
            }
            __syncthreads();  // staged tiles visible
            if (mine && wave == 0) {
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
                    for (int r = 0; r < 16; ++r) acc[cb][r] = __builtin_fmaf((float)t[r], dss, acc[cb][r]);  // :436
                }
            }
            if (mine && wave == 1) {  // P in the value dtype, dv += dO^T.P (:473-474)
                v4i pf[2];
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int w = 0; w < 4; ++w) pf[c][w] = (int)pack2<V_T>(pr[8 * c + 2 * w], pr[8 * c + 2 * w + 1]);
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int cb = 0; cb < KK; ++cb) acc[cb] = attn_mfma16<V_T>(*(const v4i*)(ot + (32 * cb + ql) * 32 + 16 * c + 8 * g), pf[c], acc[cb]);
            }
        }
    }
    if (!kok || !mine) return;
    void* dst = wave == 0 ? p.dk : p.dv;
    const int64_t oo = wave == 0 ? p.dkst.at(kv_lin, key) : p.dvst.at(kv_lin, key);
    const int ch = wave == 0 ? p.dk_ch : p.d_src;
#pragma unroll
    for (int cb = 0; cb < KK; ++cb)
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const int c0 = 32 * cb + 8 * t4 + 4 * g;
            if (c0 >= ch) continue;
#pragma unroll
            for (int u = 0; u < 4; ++u) st_rt(dst, oo + c0 + u, acc[cb][4 * t4 + u], p.grad_dtype);
        }
}

// the checks the two entry points share, in the order of attention_bwd.hip's fill_common; the operands are slices of the forward's workspace
int wide_fill_common(BwdParams& p, const void* workspace, int64_t workspace_bytes, float sm_scale, int is_causal, const void* mask, int mask_dtype,
                     int64_t ms_b, int64_t ms_h, int64_t ms_q, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len,
                     int64_t head_dim) {
    if (!workspace) return SDNQ_ERR_NULL;
    if (!shape_ok(batch, q_heads, kv_heads, q_len, kv_len, 1)) return SDNQ_ERR_SHAPE;  // (a head dim <= 0 is the next line's)
    const int dp = wide_dim(head_dim);
    if (dp == 0) return SDNQ_ERR_UNSUPPORTED;
    if (!attn_mask_ok(mask, mask_dtype)) return SDNQ_ERR_DTYPE;
    if ((uintptr_t)workspace % 256) return SDNQ_ERR_ALIGN;
    const WideWs w = wide_ws(batch, q_heads, kv_heads, q_len, kv_len, dp);
    if (workspace_bytes < w.vt) return SDNQ_ERR_SHAPE;  // qq, qs, kq, ks: the slices in front of vt
    const char* ws = (const char*)workspace;
    p.qq = (const int8_t*)(ws + w.qq); p.qs = (const float*)(ws + w.qs); p.kq = (const int8_t*)(ws + w.kq); p.ks = (const float*)(ws + w.ks);
    p.qh = q_heads; p.kh = kv_heads; p.qn = q_len; p.kn = kv_len; p.knp = (kv_len + 31) / 32 * 32;
    p.d_src = (int)head_dim; p.causal = is_causal ? 1 : 0;
    p.sm_scale = sm_scale; p.log2_sm_scale = sm_scale * ATTN_LOG2E;  // triton_atten_backward.py:88
    p.m = {mask, mask_dtype, ms_b, ms_h, ms_q};
    return SDNQ_OK;
}

template <int V_T, int DP>
void wide_bwd_launch(const BwdParams& p, int64_t heads_q, int64_t heads_k, hipStream_t s) {
    const int64_t qblocks = (p.qn + 31) / 32, kblocks = (p.kn + 31) / 32;
    if (p.dq) hipLaunchKernelGGL((attn_wide_bwd_dq_kernel<V_T, DP>), dim3((unsigned)(heads_q * qblocks)), dim3(128), 0, s, p, qblocks);
    if (p.dk || p.dv) hipLaunchKernelGGL((attn_wide_bwd_dkv_kernel<V_T, DP>), dim3((unsigned)(heads_k * kblocks)), dim3(128), 0, s, p, kblocks);
}

template <int V_T>
void wide_bwd_launch_d(const BwdParams& p, int dp, int64_t heads_q, int64_t heads_k, hipStream_t s) {
    if (dp == 160) wide_bwd_launch<V_T, 160>(p, heads_q, heads_k, s);
    else if (dp == 192) wide_bwd_launch<V_T, 192>(p, heads_q, heads_k, s);
    else if (dp == 224) wide_bwd_launch<V_T, 224>(p, heads_q, heads_k, s);
    else wide_bwd_launch<V_T, 256>(p, heads_q, heads_k, s);
}

}  // namespace

extern "C" int sdnq_hip_attn_wide_lse(const void* workspace, int64_t workspace_bytes, float sm_scale, int is_causal, const void* mask, int mask_dtype,
                                      int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q, void* lse, int lse_dtype, int64_t batch,
                                      int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len, int64_t head_dim, sdnq_stream_t stream) {
    BwdParams p{};
    const int rc = wide_fill_common(p, workspace, workspace_bytes, sm_scale, is_causal, mask, mask_dtype, mask_stride_b, mask_stride_h, mask_stride_q,
                                    batch, q_heads, kv_heads, q_len, kv_len, head_dim);
    if (rc != SDNQ_OK) return rc;
    if (!lse) return SDNQ_ERR_NULL;
    if (!float_ok(lse_dtype)) return SDNQ_ERR_DTYPE;
    p.lse = lse; p.lse_dtype = lse_dtype;
    const int64_t qblocks = (q_len + 31) / 32;
    const dim3 grid((unsigned)(batch * q_heads * qblocks)), block(64);
    hipStream_t s = (hipStream_t)stream;
    switch (wide_dim(head_dim)) {
        case 160: hipLaunchKernelGGL((attn_lse_kernel<160>), grid, block, 0, s, p, qblocks); break;
        case 192: hipLaunchKernelGGL((attn_lse_kernel<192>), grid, block, 0, s, p, qblocks); break;
        case 224: hipLaunchKernelGGL((attn_lse_kernel<224>), grid, block, 0, s, p, qblocks); break;
        default: hipLaunchKernelGGL((attn_lse_kernel<256>), grid, block, 0, s, p, qblocks); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_attn_wide_bwd(const void* workspace, int64_t workspace_bytes, const void* v, const int64_t* v_strides, int v_dtype, const void* out,
                                      const int64_t* out_strides, const void* grad, const int64_t* grad_strides, int grad_dtype, const void* grad_v,
                                      const int64_t* grad_v_strides, const void* lse, float sm_scale, int is_causal, const void* mask, int mask_dtype,
                                      int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q, float* delta, void* dq,
                                      const int64_t* dq_strides, int64_t dq_channels, void* dk, const int64_t* dk_strides, int64_t dk_channels, void* dv,
                                      const int64_t* dv_strides, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len,
                                      int64_t head_dim, sdnq_stream_t stream) {
    BwdParams p{};
    const int rc = wide_fill_common(p, workspace, workspace_bytes, sm_scale, is_causal, mask, mask_dtype, mask_stride_b, mask_stride_h, mask_stride_q,
                                    batch, q_heads, kv_heads, q_len, kv_len, head_dim);
    if (rc != SDNQ_OK) return rc;
    if (!v || !out || !grad || !grad_v || !lse || !delta) return SDNQ_ERR_NULL;
    if (v_dtype != SDNQ_BF16 && v_dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (!float_ok(grad_dtype)) return SDNQ_ERR_DTYPE;
    const int dp = wide_dim(head_dim);
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
    if (v_dtype == SDNQ_BF16) wide_bwd_launch_d<SDNQ_BF16>(p, dp, batch * q_heads, batch * kv_heads, s);
    else wide_bwd_launch_d<SDNQ_F16>(p, dp, batch * q_heads, batch * kv_heads, s);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
