// Quantized attention forward for head dims 136 .. 256 on gfx950: the default configuration of the reference's `sdnq_triton_atten`
// (kernels/triton_atten.py:540-618: int8 Q.K^T, fp32 softmax, P.V in the value dtype) where attention.hip stops at 128.  The reference pads
// such a head to the next power of two (get_attn_inputs, triton_atten.py:512-519: 160 runs as 256); here the head dim is padded to the
// next multiple of 32, DP in {160, 192, 224, 256} -- the zero channels add nothing to Q.K^T, so the scores are the same.
//
//   attn_wide_prepare_kernel <- quantize_attn (triton_atten.py:443-487): K minus its per-channel token mean (smooth_k), per-token symmetric
//                               int8 of Q and K, V laid out for the P.V operand; operand layouts as in attn_dev.h with D = DP
//   attn_wide_fwd_kernel     <- sdnq_attn_kernel (triton_atten.py:143-335) with qk_is_quantized=1, pv_is_quantized=0
//
// Work split of the forward kernel.  attention.hip's wave owns 32 queries and keeps O^T, Q and the K / V fragments in registers: at DP = 256
// that is 128 accumulator registers for O^T alone.  Here a PAIR of waves owns the 32 queries and splits the OUTPUT CHANNELS:
//   both waves compute the full S^T = K.Q^T of the tile (DP / 32 steps of the 32x32x32 i8 MFMA) and, from the same operands in the same
//   order, the same row maximum, P and row sum; each wave runs O^T = V^T.P^T for its half of the DP / 32 channel tiles only (5 tiles:
//   3 + 2, 7 tiles: 4 + 3) and writes those channels.
// So the lane-owns-query layout of attention.hip carries over (in-lane reductions, one lane exchange, per-lane alpha and 1 / l), P never
// leaves its lane, the loop has no LDS traffic and no barrier, and a wave holds half the O^T accumulators and half the V fragments.  The
// price is the score arithmetic twice.  A workgroup is two pairs: two query tiles of one head, which stream the same K / V.
// Software pipeline: K of block kb + 1 is in registers and S(kb + 1) on the matrix pipe while the VALU works on the scores of kb; the key
// scales and V of kb + 1 are loaded as soon as block kb has consumed its own.
#include "attn_wide_dev.h"

namespace {

// wide_dim, the workspace layout wide_ws and the channel-slot constants: attn_wide_dev.h (shared with attention_wide_bwd.hip)

// ---- channel sums of K: thread tid adds channels [8 (tid % 32), + 8) of the rows lo + tid / 32, + 8, ... below hi --------------------------
template <int T_ID>
__device__ __forceinline__ void wide_row_sums(const uint16_t* __restrict__ khead, int64_t stride, int64_t lo, int64_t hi, int d_src, float (&acc)[8]) {
    const int c8 = ((int)threadIdx.x & 31) * 8;
    for (int64_t r = lo + ((int)threadIdx.x >> 5); r < hi; r += 8) {
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (c8 < d_src) Vec16<T_ID>::unpack(*(const uint4*)(khead + r * stride + c8), v);  // channels past d_src: zero padding
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
}
// ... and the workgroup's sum of channel tid, the 8 row groups added in a fixed order.  red: 256 * 8 floats of LDS.
__device__ __forceinline__ float wide_channel_sum(const float (&acc)[8], float* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[e];
    __syncthreads();
    float s = 0.0f;
    for (int r = 0; r < 8; ++r) s += red[(r * 32 + (tid >> 3)) * 8 + (tid & 7)];
    return s;
}

// ---- per-token int8 quantization of [heads][n_src][d_src] into dp channels (32 lanes per token), optional mean subtraction ---------------
// As attn_quant_block (attention.hip): n_dst >= n_src token slots per head, the extra tokens get zero codes and a zero scale.
template <int T_ID>
__device__ __forceinline__ void wide_quant_block(const void* __restrict__ x, const Strides xst, const float* mean, int8_t* __restrict__ xq, float* __restrict__ xs,
                                                 int64_t heads, int64_t n_src, int64_t n_dst, int dp, int d_src, bool frag_major, int64_t block) {
    const int64_t t = block * 256 + threadIdx.x;
    const int64_t row = t >> 5;
    const int c8 = (int)(t & 31) * 8;
    const bool live = row < heads * n_dst;
    int64_t head = 0, n = 0;
    if (live) divmod(row, n_dst, head, n);
    const bool real = live && n < n_src;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (real && c8 < d_src) Vec16<T_ID>::unpack(*(const uint4*)((const uint16_t*)x + xst.at(head, n) + c8), v);
    if (mean != nullptr && real && c8 < d_src) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] -= mean[c8 + e];  // k.to(float32).sub_(mean), triton_atten.py:459-463
    }
    float amax = attn_row_amax(v, 16);
    amax = fmaxf(amax, lane_xor(amax, 16));
    u32 o[2];
    const float scale = attn_quant8_amax(v, amax, o);  // quantize_int_mm, quant_utils.py:265-273: the codes of attention.hip's quantizer
    if (live && c8 < dp) {
        if (frag_major) *(uint2*)(xq + head * n_dst * dp + attn_kfrag_offset(n, c8, dp)) = make_uint2(o[0], o[1]);  // (n_dst is a multiple of 32)
        else *(uint2*)(xq + row * dp + c8) = make_uint2(o[0], o[1]);
        if (c8 == 0) xs[row] = scale;
    }
}

// ---- V [heads][kn][d_src] -> P.V operand in MFMA-fragment order with dp channels (attn_vt_block's layout, attn_dev.h) -------------------
__device__ __forceinline__ void wide_vt_block(const uint16_t* __restrict__ v, const Strides vst, uint16_t* __restrict__ vt, int64_t kn, int64_t knp, int dp, int d_src,
                                              int64_t head, int64_t kb, uint16_t (*tile)[WIDE_SLOTS + 2]) {
    const int64_t key0 = kb * 32;
    const int kkn = dp / 32;
    uint16_t* dst = vt + (head * (knp / 32) + kb) * (int64_t)(kkn * 2 * 512);
    const uint16_t* vhead = v + vst.at(head, 0);
    for (int t = threadIdx.x; t < 32 * 32; t += 256) {
        const int kr = t >> 5, c8 = (t & 31) * 8;
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

struct WidePrep {
    const void *q, *k, *v;
    int8_t *qq, *kq;
    float *qs, *ks;
    uint16_t* vt;
    Strides qst, kst, vst;
    const float* kpart;  // [kheads][WIDE_KMEAN_SPLITS][256] channel sums (smooth_k over a long key sequence) or nullptr
    float* kpart_out;    // the same table, written by the channel-sum section of a launch
    int64_t qheads, kheads, qn, kn, knp, nqb, nkb, nvb, nmb;  // workgroups per section: Q rows, K rows, V tiles, K channel sums
    int dp, d_src;
    bool smooth_inline;  // K means computed inside the K workgroups (short key sequences)
};

// one launch, four kinds of workgroup, as attn_prepare_kernel (attention.hip): [0, nqb) quantize Q (8 tokens each), the next nkb quantize K
// (8 tokens; knp is a multiple of 32, so a workgroup never straddles heads), the next nvb lay out V, the last nmb sum K's channels over a
// token split.  With smooth_k over more than 256 keys the K rows wait for the channel sums: the host launches {Q, V, sums} and then {K}.
template <int T_ID>
__global__ __launch_bounds__(256) void attn_wide_prepare_kernel(const WidePrep p) {
    __shared__ float smean[WIDE_SLOTS];
    __shared__ __attribute__((aligned(16))) uint16_t tile[32][WIDE_SLOTS + 2];
    float* red = (float*)&tile[0][0];  // 256 * 8 floats <= sizeof(tile)
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    if (b < p.nqb) {
        wide_quant_block<T_ID>(p.q, p.qst, nullptr, p.qq, p.qs, p.qheads, p.qn, p.qn, p.dp, p.d_src, false, b);
    } else if (b < p.nqb + p.nkb) {
        const int64_t kb = b - p.nqb;
        const float* mean = nullptr;
        if (p.smooth_inline || p.kpart != nullptr) {
            int64_t head, rem;
            divmod(kb * 8, p.knp, head, rem);
            float s = 0.0f;
            if (p.smooth_inline) {  // every K workgroup sums its head's channels itself
                float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                wide_row_sums<T_ID>((const uint16_t*)p.k + p.kst.at(head, 0), p.kst.n, 0, p.kn, p.d_src, acc);
                s = wide_channel_sum(acc, red);
            } else {
                const float* pp = p.kpart + head * WIDE_KMEAN_SPLITS * WIDE_SLOTS + tid;
                for (int i = 0; i < WIDE_KMEAN_SPLITS; ++i) s += pp[i * WIDE_SLOTS];
            }
            smean[tid] = s / (float)p.kn;  // k.mean(dim=2), triton_atten.py:459
            __syncthreads();
            mean = smean;
        }
        wide_quant_block<T_ID>(p.k, p.kst, mean, p.kq, p.ks, p.kheads, p.kn, p.knp, p.dp, p.d_src, true, kb);
    } else if (b < p.nqb + p.nkb + p.nvb) {
        int64_t vhead, vblk;
        divmod(b - p.nqb - p.nkb, p.knp >> 5, vhead, vblk);
        wide_vt_block((const uint16_t*)p.v, p.vst, p.vt, p.kn, p.knp, p.dp, p.d_src, vhead, vblk, tile);
    } else {
        const int64_t blk = b - p.nqb - p.nkb - p.nvb;
        const int64_t head = blk / WIDE_KMEAN_SPLITS, split = blk % WIDE_KMEAN_SPLITS;
        const int64_t per = (p.kn + WIDE_KMEAN_SPLITS - 1) / WIDE_KMEAN_SPLITS, lo = split * per, hi = lo + per < p.kn ? lo + per : p.kn;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        wide_row_sums<T_ID>((const uint16_t*)p.k + p.kst.at(head, 0), p.kst.n, lo, hi, p.d_src, acc);
        p.kpart_out[blk * WIDE_SLOTS + tid] = wide_channel_sum(acc, red);
    }
}

struct WideParams {
    const int8_t* qq; const float* qs; const int8_t* kq; const float* ks; const uint16_t* vt;
    void* out;
    int64_t qh, kh, qn, kn, knp;
    int qblocks;  // workgroups per head: two query tiles each
    float log2_sm_scale;
    Strides ost;  // output strides (elements)
    int d_out;    // channels the output tensor has (<= DP)
    AttnMask m;
};

// ---- forward: one wave PAIR = 32 queries of one head, wave `half` of the pair owns the channel tiles [half * NT, ...); 2 pairs per workgroup ----
// The score arithmetic, the masks (only in the one block that needs them: key tail, causal diagonal; every block under a user mask), the
// lazy row maximum and the rescale of O only when a row maximum of the wave moved are those of attn_fwd_kernel (attention.hip).
template <int V_T, int OUT_T, int DP, bool CAUSAL, bool HAS_MASK>
__global__ __launch_bounds__(256) void attn_wide_fwd_kernel(const WideParams p) {
    SDNQ_KERNARGS_NOW("s"(p.qq), "s"(p.qs), "s"(p.kq), "s"(p.ks), "s"(p.vt), "s"(p.out), "s"(p.qh), "s"(p.kh), "s"(p.qn), "s"(p.kn), "s"(p.knp), "s"(p.qblocks),
                      "s"(p.log2_sm_scale), "s"(p.ost.b), "s"(p.ost.h), "s"(p.ost.n), "s"(p.ost.heads), "s"(p.d_out), "s"(p.m.mask), "s"(p.m.mask_dtype),
                      "s"(p.m.ms_z), "s"(p.m.ms_h), "s"(p.m.ms_q));
    constexpr int KK = DP / 32;        // int8 MFMA K steps of Q.K^T; also the 32-channel tiles of O
    constexpr int NT = (KK + 1) / 2;   // channel tiles of the pair's first wave; the second has KK - NT (one fewer when KK is odd)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ql = lane & 31, g = lane >> 5;
    const int half = wave & 1, t0 = half * NT;  // wave-uniform: this wave's first channel tile
    auto owns = [&](int dd) { return KK % 2 == 0 || dd + 1 < NT || half == 0; };  // tile t0 + dd exists (wave-uniform)
    // workgroup b runs on XCD b % 8 (private L2 each): every XCD gets a contiguous range of the (head, query block) sequence, so the query
    // blocks of one head, which stream the same K / V, share one L2 (as attention.hip)
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = bid % 8, j = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    }
    const int64_t head_lin = bid / p.qblocks;  // z * QH + h
    const int qblk = bid % p.qblocks;
    const int64_t q0 = ((int64_t)qblk * 2 + (wave >> 1)) * 32;
    if (q0 >= p.qn) return;  // wave-uniform, and the kernel has no barrier
    int64_t z, h;
    divmod(head_lin, p.qh, z, h);
    int64_t kvh, kvr;
    divmod(h * p.kh, p.qh, kvh, kvr);
    const int64_t kv_lin = z * p.kh + kvh;  // offset_k of triton_atten.py:212 (grouped-query mapping)
    const int64_t qi = q0 + ql, qrow = qi < p.qn ? qi : p.qn - 1;

    // every load goes through a buffer descriptor: head base in SGPRs, constant per-lane offset, block offset in the scalar operand
    auto rsQ = SDNQ_MAKE_RSRC(p.qq + head_lin * p.qn * DP);
    auto rsK = SDNQ_MAKE_RSRC(p.kq + kv_lin * p.knp * DP);
    auto rsV = SDNQ_MAKE_RSRC(p.vt + kv_lin * p.knp * DP);
    auto rsS = SDNQ_MAKE_RSRC(p.ks + kv_lin * p.knp);
    const int lofs = lane * 16, sofs = 32 * g;  // byte offsets of this lane inside a fragment tile / a block's 32 k_scales
    v4i qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[kk] = SDNQ_BUF_LOAD16(rsQ, (int)qrow * DP + 16 * g, 32 * kk);
    // ((acc * q_scale) * k_scale) * log2_sm_scale of triton_atten.py:264 as acc * (k_scale * (q_scale * log2_sm_scale))
    const float qsl = p.qs[head_lin * p.qn + qrow] * p.log2_sm_scale;

    v16f o[NT];
#pragma unroll
    for (int dd = 0; dd < NT; ++dd)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dd][r] = 0.0f;
    float m_i = -__builtin_inff();
    v2f l2 = {0.0f, 0.0f};  // this lane's half of the row sum (16 of every 32 keys), two partial sums

    auto load_k = [&](int kb, v4i (&kf)[KK]) {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kf[kk] = SDNQ_BUF_LOAD16(rsK, lofs, kb * (KK * 1024) + kk * 1024);
    };
    auto load_v = [&](int kb, v4i (&vf)[NT][2]) {  // this wave's channel tiles only
#pragma unroll
        for (int dd = 0; dd < NT; ++dd)
            if (owns(dd)) {
#pragma unroll
                for (int c = 0; c < 2; ++c) vf[dd][c] = SDNQ_BUF_LOAD16(rsV, lofs, kb * (KK * 2048) + ((t0 + dd) * 2 + c) * 1024);
            }
    };
    auto load_s = [&](int kb, v4f (&ks)[4]) {  // registers 8c..8c+7 <-> keys key0 + 16c + 8g + 0..7 (k_scale rows are padded to knp)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            ks[2 * c] = __builtin_bit_cast(v4f, SDNQ_BUF_LOAD16(rsS, sofs, kb * 128 + 64 * c));
            ks[2 * c + 1] = __builtin_bit_cast(v4f, SDNQ_BUF_LOAD16(rsS, sofs, kb * 128 + 64 * c + 16));
        }
    };
    auto qk_mfma = [&](const v4i (&kf)[KK]) {
        v16i s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf[kk], qf[kk], s, 0, 0, 0);
        return s;
    };
    // block kb from its scores `s`, key scales `ks` and V fragments `vf`; `next` >= 0: the block whose key scales and V are loaded into
    // `ks` / `vf` as soon as this block has read them
    auto softmax_pv = [&](const v16i& s, v4f (&ks)[4], v4i (&vf)[NT][2], int kb, int next, auto maskedc) {
        constexpr bool MASKED = decltype(maskedc)::value;
        const int64_t key0 = (int64_t)kb * 32;
        // t = acc * k_scale; the per-query factor qsl >= 0 commutes with the row maximum, so it is applied inside the fma that also
        // subtracts the maximum: p = exp2(t * qsl - m)
        v2f t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const v4f k4 = ks[j >> 1];
            t[j] = (v2f){(float)s[2 * j], (float)s[2 * j + 1]} * (v2f){k4[2 * (j & 1)], k4[2 * (j & 1) + 1]};
        }
        if (next >= 0) load_s(next, ks);
        float alpha;
        v2f psum = {0.0f, 0.0f};
        if constexpr (MASKED) {
            // fully scaled scores first, then the masks, and the -inf-safe updates of triton_atten.py:282-285 (a row that has seen no
            // visible key yet keeps m = -inf, alpha = 1, p = 0)
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] *= qsl;
            const char* mrow = nullptr;
            if constexpr (HAS_MASK) {
                const int64_t mq = qi < p.qn ? qi : p.qn - 1;
                mrow = (const char*)p.m.mask + (z * p.m.ms_z + h * p.m.ms_h + mq * p.m.ms_q) * (p.m.mask_dtype == -1 ? 1 : (p.m.mask_dtype == SDNQ_F32 ? 4 : 2));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t key = key0 + 16 * (r >> 3) + 8 * g + (r & 7);
                bool ok = key < p.kn;              // triton_atten.py:280-281
                if (CAUSAL) ok = ok && key <= qi;  // :273-274
                float add = 0.0f;
                if constexpr (HAS_MASK) {
                    if (ok) {
                        if (p.m.mask_dtype == -1) ok = ((const int8_t*)mrow)[key] != 0;  // :276-277
                        else add = ld_rt(mrow, key, p.m.mask_dtype);                   // :278-279 (added as is)
                    }
                }
                t[r >> 1][r & 1] = ok ? t[r >> 1][r & 1] + add : -__builtin_inff();
            }
            float m_blk = fmaxf(t[0][0], t[0][1]);
#pragma unroll
            for (int j = 1; j < 8; ++j) m_blk = fmaxf(fmaxf(m_blk, t[j][0]), t[j][1]);
            m_blk = attn_max32(m_blk);
            const float m_new = fmaxf(m_i, m_blk);
            const bool dead = m_new == -__builtin_inff();
            alpha = dead ? 1.0f : __builtin_amdgcn_exp2f(m_i - m_new);
            m_i = m_new;
            const float m_use = dead ? 0.0f : m_new;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                t[j] -= m_use;
                t[j] = (v2f){__builtin_amdgcn_exp2f(t[j][0]), __builtin_amdgcn_exp2f(t[j][1])};
                psum += t[j];
            }
        } else {
            float m_blk = fmaxf(t[0][0], t[0][1]);
#pragma unroll
            for (int j = 1; j < 8; ++j) m_blk = fmaxf(fmaxf(m_blk, t[j][0]), t[j][1]);
            m_blk = attn_max32(m_blk);  // the other 16 keys of this query live in lane ^ 32
            // lazy reference maximum (attention.hip): m_i follows the row maximum only when it grew by more than 2^8 for some query of the
            // wave; otherwise p <= 2^8, alpha = 1 and O is not rescaled.  o / l is the same quotient either way.
            const float m_cand = m_blk * qsl;  // finite: every key of a plain block is visible
            alpha = 1.0f;
            if (__builtin_amdgcn_ballot_w64(m_cand > m_i + 8.0f) != 0) {
                const float m_new = fmaxf(m_i, m_cand);
                alpha = __builtin_amdgcn_exp2f(m_i - m_new);
                m_i = m_new;
            }
            const v2f qsl2 = {qsl, qsl}, mneg2 = {-m_i, -m_i};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                t[j] = __builtin_elementwise_fma(t[j], qsl2, mneg2);
                t[j] = (v2f){__builtin_amdgcn_exp2f(t[j][0]), __builtin_amdgcn_exp2f(t[j][1])};
                psum += t[j];
            }
        }
        l2 = l2 * alpha + psum;  // l_i = fma(l_i, alpha, sum(p)), :291
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
            for (int dd = 0; dd < NT; ++dd) o[dd] *= alpha;
        }
        // P in the value dtype (p.to(v.dtype), :320), packed as the second MFMA operand: 8 keys per lane group and K step
        v4i pf[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if constexpr (V_T == SDNQ_BF16) pf[c][w] = __builtin_bit_cast(int, __builtin_convertvector(t[4 * c + w], v2bf));
                else pf[c][w] = __builtin_bit_cast(int, __builtin_convertvector(t[4 * c + w], v2h));
            }
        // key step outermost: consecutive MFMAs write different accumulators
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int dd = 0; dd < NT; ++dd)
                if (owns(dd)) o[dd] = attn_mfma16<V_T>(vf[dd][c], pf[c], o[dd]);
        if (next >= 0) load_v(next, vf);
    };

    // blocks [0, n_plain) need no mask; at most ONE more block does (the key tail, or the causal diagonal block key0 == q0); with an
    // attention mask every block takes the masked path
    int nkb = (int)((p.kn + 31) / 32), n_plain = (int)(p.kn / 32);
    if (CAUSAL) {
        const int lim = (int)(q0 / 32) + 1;  // blocks past the last query of this tile are fully masked (triton_atten.py:245)
        nkb = nkb < lim ? nkb : lim;
        n_plain = n_plain < lim - 1 ? n_plain : lim - 1;
    }
    if (HAS_MASK) n_plain = 0;
    v4i kf[KK], vf[NT][2];
    v4f ks[4];
    if (n_plain > 0) {
        const int last = n_plain - 1;
        v16i sA, sB;
        load_k(0, kf);
        load_s(0, ks);
        load_v(0, vf);
        sA = qk_mfma(kf);
        load_k(1 < last ? 1 : last, kf);
        // two blocks per trip so that the score registers swap roles without moves
#pragma nounroll
        for (int kb = 0; kb < n_plain; kb += 2) {
            // block kb: scores in sA, scales / V in ks / vf; K(kb+1) in kf
            sB = qk_mfma(kf);
            load_k(kb + 2 < last ? kb + 2 : last, kf);
            softmax_pv(sA, ks, vf, kb, kb + 1 < last ? kb + 1 : last, std::false_type{});
            if (kb + 1 >= n_plain) break;
            sA = qk_mfma(kf);
            load_k(kb + 3 < last ? kb + 3 : last, kf);
            softmax_pv(sB, ks, vf, kb + 1, kb + 2 < last ? kb + 2 : last, std::false_type{});
        }
    }
#pragma nounroll
    for (int kb = n_plain; kb < nkb; ++kb) {
        load_k(kb, kf);
        load_s(kb, ks);
        load_v(kb, vf);
        const v16i s = qk_mfma(kf);
        softmax_pv(s, ks, vf, kb, -1, std::true_type{});
    }
    if (qi >= p.qn) return;
    float l_i = l2[0] + l2[1];
    l_i += __shfl_xor(l_i, 32);
    const float inv = l_i > 0.0f ? 1.0f / l_i : 0.0f;  // acc *= fdiv(1.0, l_i), :324; a row with no visible key is 0
    char* orow = (char*)p.out + p.ost.at(head_lin, qi) * FT<OUT_T>::bytes;
#pragma unroll
    for (int dd = 0; dd < NT; ++dd)
        if (owns(dd)) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int dcol = 32 * (t0 + dd) + 8 * t + 4 * g;  // registers 4t..4t+3 are 4 consecutive channels
                if (dcol >= p.d_out) continue;
                float f[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) f[u] = o[dd][4 * t + u] * inv;
                if constexpr (OUT_T == SDNQ_F32) {
                    *(float4*)(orow + dcol * 4) = make_float4(f[0], f[1], f[2], f[3]);
                } else {
                    const u32 lo = FT<OUT_T>::bits(f[0]) | ((u32)FT<OUT_T>::bits(f[1]) << 16);
                    const u32 hi = FT<OUT_T>::bits(f[2]) | ((u32)FT<OUT_T>::bits(f[3]) << 16);
                    *(uint2*)(orow + dcol * 2) = make_uint2(lo, hi);
                }
            }
        }
}

template <int V_T, int OUT_T, int DP>
int wide_launch(const WideParams& p, int causal, int64_t blocks, hipStream_t s) {
    const dim3 grid((unsigned)blocks), block(256);
    if (p.m.mask) {
        if (causal) hipLaunchKernelGGL((attn_wide_fwd_kernel<V_T, OUT_T, DP, true, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attn_wide_fwd_kernel<V_T, OUT_T, DP, false, true>), grid, block, 0, s, p);
    } else {
        if (causal) hipLaunchKernelGGL((attn_wide_fwd_kernel<V_T, OUT_T, DP, true, false>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attn_wide_fwd_kernel<V_T, OUT_T, DP, false, false>), grid, block, 0, s, p);
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

template <int V_T, int OUT_T>
int wide_launch_d(const WideParams& p, int dp, int causal, int64_t blocks, hipStream_t s) {
    if (dp == 160) return wide_launch<V_T, OUT_T, 160>(p, causal, blocks, s);
    if (dp == 192) return wide_launch<V_T, OUT_T, 192>(p, causal, blocks, s);
    if (dp == 224) return wide_launch<V_T, OUT_T, 224>(p, causal, blocks, s);
    if (dp == 256) return wide_launch<V_T, OUT_T, 256>(p, causal, blocks, s);
    return SDNQ_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int64_t sdnq_hip_attn_wide_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len, int64_t head_dim,
                                                      int hadamard_group) {
    if (!shape_ok(batch, q_heads, kv_heads, q_len, kv_len, head_dim)) return SDNQ_ERR_SHAPE;
    const int dp = wide_dim(head_dim);
    if (dp == 0 || hadamard_group != 0) return SDNQ_ERR_UNSUPPORTED;
    return wide_ws(batch, q_heads, kv_heads, q_len, kv_len, dp).total;
}

extern "C" int sdnq_hip_attn_wide(const void* q, const void* k, const void* v, int dtype, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                  int64_t q_len, int64_t kv_len, int64_t head_dim, const int64_t* q_strides, const int64_t* k_strides,
                                  const int64_t* v_strides, int smooth_k, int hadamard_group, float sm_scale, int is_causal, const void* mask,
                                  int mask_dtype, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q, void* out, int out_dtype,
                                  const int64_t* out_strides, void* workspace, int64_t workspace_bytes, sdnq_stream_t stream) {
    if (!q || !k || !v || !out || !workspace) return SDNQ_ERR_NULL;
    if (!shape_ok(batch, q_heads, kv_heads, q_len, kv_len, head_dim)) return SDNQ_ERR_SHAPE;
    const int dp = wide_dim(head_dim);
    if (dp == 0 || hadamard_group != 0 || (dtype != SDNQ_BF16 && dtype != SDNQ_F16)) return SDNQ_ERR_UNSUPPORTED;
    if (!attn_mask_ok(mask, mask_dtype) || (out_dtype != dtype && out_dtype != SDNQ_F32)) return SDNQ_ERR_DTYPE;
    const WideWs w = wide_ws(batch, q_heads, kv_heads, q_len, kv_len, dp);
    if (workspace_bytes < w.total) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 || (uintptr_t)out % 8 || (uintptr_t)workspace % 256) return SDNQ_ERR_ALIGN;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int64_t qheads = batch * q_heads, kheads = batch * kv_heads, knp = (kv_len + 31) / 32 * 32;

    WidePrep pp{};
    pp.q = q; pp.k = k; pp.v = v;
    pp.qq = (int8_t*)(ws + w.qq); pp.qs = (float*)(ws + w.qs); pp.kq = (int8_t*)(ws + w.kq); pp.ks = (float*)(ws + w.ks); pp.vt = (uint16_t*)(ws + w.vt);
    if (!attn_set_strides(q_strides, q_heads, q_len, head_dim, pp.qst) || !attn_set_strides(k_strides, kv_heads, kv_len, head_dim, pp.kst) ||
        !attn_set_strides(v_strides, kv_heads, kv_len, head_dim, pp.vst))
        return SDNQ_ERR_ALIGN;
    WideParams fp{};
    if (!attn_set_strides(out_strides, q_heads, q_len, head_dim, fp.ost, 4)) return SDNQ_ERR_ALIGN;  // 8-byte groups of 4 channels
    pp.smooth_inline = smooth_k && kv_len <= 256;
    pp.kpart = (smooth_k && !pp.smooth_inline) ? (const float*)(ws + w.kmean) : nullptr;
    pp.kpart_out = (float*)(ws + w.kmean);
    pp.qheads = qheads; pp.kheads = kheads; pp.qn = q_len; pp.kn = kv_len; pp.knp = knp; pp.dp = dp; pp.d_src = (int)head_dim;
    pp.nqb = (qheads * q_len + 7) / 8;
    pp.nkb = kheads * knp / 8;  // exact: knp is a multiple of 32
    pp.nvb = kheads * (knp / 32);
    pp.nmb = 0;
    auto prepare = [&](const WidePrep& a) {
        const dim3 grid((unsigned)(a.nqb + a.nkb + a.nvb + a.nmb)), block(256);
        if (dtype == SDNQ_BF16) hipLaunchKernelGGL((attn_wide_prepare_kernel<SDNQ_BF16>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((attn_wide_prepare_kernel<SDNQ_F16>), grid, block, 0, s, a);
    };
    if (pp.kpart) {
        WidePrep first = pp, second = pp;
        first.nkb = 0; first.nmb = kheads * WIDE_KMEAN_SPLITS;  // everything that does not need the means, next to the channel sums
        second.nqb = 0; second.nvb = 0;                          // then the K rows
        prepare(first);
        prepare(second);
    } else {
        prepare(pp);
    }
    SDNQ_CHECK_LAUNCH();

    fp.qq = pp.qq; fp.qs = pp.qs; fp.kq = pp.kq; fp.ks = pp.ks; fp.vt = pp.vt; fp.out = out;
    fp.qh = q_heads; fp.kh = kv_heads; fp.qn = q_len; fp.kn = kv_len; fp.knp = knp;
    fp.qblocks = (int)((q_len + 63) / 64);
    fp.log2_sm_scale = sm_scale * ATTN_LOG2E;
    fp.d_out = (int)head_dim;
    fp.m = {mask, mask_dtype, mask_stride_b, mask_stride_h, mask_stride_q};
    const int64_t blocks = qheads * fp.qblocks;
#define WIDE_CASE(VT, OT) if (dtype == VT && out_dtype == OT) return wide_launch_d<VT, OT>(fp, dp, is_causal, blocks, s)
    WIDE_CASE(SDNQ_BF16, SDNQ_BF16);
    WIDE_CASE(SDNQ_BF16, SDNQ_F32);
    WIDE_CASE(SDNQ_F16, SDNQ_F16);
    WIDE_CASE(SDNQ_F16, SDNQ_F32);
#undef WIDE_CASE
    return SDNQ_ERR_DTYPE;
}
