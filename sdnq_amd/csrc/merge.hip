// Merging a low-rank adapter into the stored codes of a frozen quantized Linear weight: codes -> codes in ONE launch.  No reference
// interface: the reference has no adapters; this replaces what a user of it composes per layer -- dequantize to a float [N][K] matrix,
// addmm the delta scale * up . down, quantize again (about five passes over 4 N K bytes) -- by one read of the codes and one write of
// the merged codes and scales.  Nothing of size N x K in float ever exists.
//
//   sdnq_hip_merge_lowrank   e = fmaf(scale, sum_r up[n][r] down[r][k], w32[n][k]), then e = row_scale[n] * e where row_scale is given (DoRA's
//       c), all float32 and as dora.hip's norm kernel defines them: w32 is dequant16's value (weight_dev.h) of the stored codes, the rank
//       product runs on v_mfma_f32_16x16x32 in rank steps of 32.  e is then quantized with the arithmetic of quantize.hip (quant_dev.h has
//       what the two units share): per (row, group) min / max / amax -> scale (and zero point), q = e / s or (e - zp) / s, round half to even
//       and clamp (floats: nan_to_num, clamp, convert), the reference's packing.
//       The kernel has the norm kernel's shape: a workgroup (4 waves) owns 16 rows and walks K -- or, where the rows alone would leave CUs
//       idle, its share blockIdx.y of K -- in chunks of MG_KC = 256: wave w takes the 64
//       columns 64 w .. of the chunk, its lane (li = lane % 16, g = lane / 16) the 16-run k0 = chunk + 64 w + 16 g of row n0 + li.  down is
//       staged per 32-rank step in LDS as it lies in memory and read by ds_read_b64_tr_b16 (rows of 528 bytes: a 32-lane half's transposed
//       read is 2-way conflicted -- dora.hip's layout, worked out by hand there, not measured).  EXEC is full at those reads and at every
//       cross-lane step below: the branches around them are workgroup-uniform, rows / runs outside the matrix are computed on zeros, take
//       part in the reductions with the identities (+inf, -inf, 0) and store nothing.
//       How a group's statistics cross lanes (MODE):
//         0  group 16 / 32 / 64: the group lies in 1 / 2 / 4 lanes of one wave (lanes li, li + 16, li + 32, li + 48 hold one row):
//            __shfl_xor by 16 and 32.  One sweep over K.
//         1  group 128 / 256: two / four waves' 64 columns; each wave's row statistics go through LDS (st), two barriers per chunk.  One sweep.
//         2  row-wise (group == K, any K): two sweeps.  The first keeps running statistics per lane, which are then joined over the row's 16
//            lanes (shuffles, then LDS); the second computes e again -- the same loop body, the same operations on the same operands, hence
//            the same bits -- and encodes.  Twice the matrix-core work and twice the reads of the codes and of down; with K shared out
//            over several workgroups each of them makes the first sweep over ALL of K and the second over its share.
//       min / max do not depend on the order of their operands, so every route gives the quantizer's statistics bit for bit.  A lane's 16
//       codes go through an LDS row of its own (the packers index them by a table: registers would become scratch), as in quant_pack_kernel.
//       One launch, no atomics, no workspace, the same bits on every call, capturable.  Untuned beyond the share of K per workgroup.
#include "quant_dev.h"
#include "weight_dev.h"

namespace {

typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s* lds_v4s_ptr;

template <bool IS_BF16>
__device__ __forceinline__ v4f mfma16(v4i a, v4i b, v4f c) {
    if constexpr (IS_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

constexpr int MG_KC = 256;   // columns of K per workgroup iteration (64 per wave)
constexpr int MG_ROW = 528;  // bytes per LDS row of the staged rank step: 256 16-bit columns + 16

__device__ __forceinline__ void stat16(const float (&x)[16], float& lo, float& hi, float& amax) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        lo = fminf(lo, x[j]);
        hi = fmaxf(hi, x[j]);
        amax = fmaxf(amax, fabsf(x[j]));
    }
}

// quant_stats_kernel's last step (quantize.hip): the scale and zero point of a group from its statistics
__device__ __forceinline__ void group_scale(bool asym, float lo, float hi, float amax, float qmin, float qmax, float& s, float& zp) {
    if (asym) {
        s = (hi - lo) / (qmax - qmin);
        zp = (qmin == 0.0f) ? lo : lo - s * qmin;
    } else {
        s = amax / qmax;
        zp = 0.0f;
    }
}

template <bool IS_BF16, int MODE>
__global__ __launch_bounds__(256) void merge_lowrank_kernel(const DeqParams p, const QuantParams o, const PackTable t,
                                                            const uint16_t* __restrict__ up, const uint16_t* __restrict__ down, int R,
                                                            float scale, const float* __restrict__ row_scale, int cpw) {
    __shared__ __attribute__((aligned(16))) uint8_t img[32 * MG_ROW];  // [rank of the step][k of the chunk]
    __shared__ u32 codes[256][17];                                     // a lane's 16 codes, for the table-driven packers
    __shared__ float st[3][4][16];                                     // [lo, hi, amax][wave][li]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15, q = (lane >> 2) & 3, pp = lane & 3;
    const int64_t n = (int64_t)blockIdx.x * 16 + li;
    const bool n_ok = n < p.N;
    const bool lowrank = up != nullptr;  // workgroup-uniform
    const float rsv = (row_scale && n_ok) ? row_scale[n] : 1.0f;
    const WeightFmt f = o.fmt;
    const bool asym = (f.kind == SDNQ_KIND_UINT || f.kind == SDNQ_KIND_UFLOAT);
    const bool is_int = (f.kind == SDNQ_KIND_INT || f.kind == SDNQ_KIND_UINT);
    const bool packed = (f.storage == SDNQ_ST_PACKED_U8 || f.storage == SDNQ_ST_PACKED_I16);
    const int gs = p.group_size;
    const v4i zero = {0, 0, 0, 0};
    float lo = __builtin_inff(), hi = -__builtin_inff(), amax = 0.0f;  // MODE 2: the lane's running statistics of its row
    float s = 0.0f, zp = 0.0f;
    // blockIdx.y: the workgroup's share of the chunks, cpw of them from kbeg (the groups of a chunk need nothing of another chunk)
    const int64_t kbeg = (int64_t)blockIdx.y * cpw * MG_KC;
    const int64_t kend = kbeg + (int64_t)cpw * MG_KC < p.K ? kbeg + (int64_t)cpw * MG_KC : p.K;
    for (int sweep = 0; sweep < (MODE == 2 ? 2 : 1); ++sweep) {
        const bool stats_only = MODE == 2 && sweep == 0;
        if (MODE == 2 && sweep == 1) {
            lo = fminf(lo, __shfl_xor(lo, 16, 64)); hi = fmaxf(hi, __shfl_xor(hi, 16, 64)); amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
            lo = fminf(lo, __shfl_xor(lo, 32, 64)); hi = fmaxf(hi, __shfl_xor(hi, 32, 64)); amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
            if (g == 0) { st[0][wave][li] = lo; st[1][wave][li] = hi; st[2][wave][li] = amax; }
            __syncthreads();
            lo = fminf(fminf(st[0][0][li], st[0][1][li]), fminf(st[0][2][li], st[0][3][li]));
            hi = fmaxf(fmaxf(st[1][0][li], st[1][1][li]), fmaxf(st[1][2][li], st[1][3][li]));
            amax = fmaxf(fmaxf(st[2][0][li], st[2][1][li]), fmaxf(st[2][2][li], st[2][3][li]));
            group_scale(asym, lo, hi, amax, o.qmin, o.qmax, s, zp);
            if (tid < 16 && n_ok && blockIdx.y == 0) {
                o.scale[n] = s;
                if (asym) o.zp[n] = zp;
            }
        }
        // the statistics of a row-wise weight need the whole row: every workgroup of the row sweeps all of K for them
        const int64_t klo = stats_only ? 0 : kbeg, khi = stats_only ? p.K : kend;
        for (int64_t kb = klo; kb < khi; kb += MG_KC) {
            const int64_t k0 = kb + 64 * wave + 16 * g;
            const bool run = n_ok && k0 < p.K;  // K % 16 == 0: a run of 16 never leaves its row
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = 0.0f;
            if (run) dequant16(p, n, k0, v);
            v4f acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
            if (lowrank) {
                for (int rs = 0; rs < R; rs += 32) {
                    // the step's global loads go out before the barrier, beside the loads of the codes (as in dora.hip)
                    v4i d[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int oo = tid + 256 * i, r = oo >> 5, ch = oo & 31;
                        const int64_t kk = kb + 8 * ch;
                        d[i] = (rs + r < R && kk < p.K) ? *(const v4i*)(down + (int64_t)(rs + r) * p.K + kk) : zero;
                    }
                    const int rc = rs + 8 * g;  // rank % 8 == 0: a chunk is inside the row of up or past it
                    const v4i fb = (n_ok && rc < R) ? *(const v4i*)(up + n * R + rc) : zero;
                    __syncthreads();  // the reads of the step before are done
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int oo = tid + 256 * i, r = oo >> 5, ch = oo & 31;
                        *(v4i*)(img + r * MG_ROW + 16 * ch) = d[i];
                    }
                    __syncthreads();
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint8_t* a0 = img + (8 * g + q) * MG_ROW + 2 * (64 * wave + 16 * pp + 4 * j);
                        const v4s l4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_ptr)a0);
                        const v4s h4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_ptr)(a0 + 4 * MG_ROW));
                        const v2i l2 = __builtin_bit_cast(v2i, l4), h2 = __builtin_bit_cast(v2i, h4);
                        acc[j] = mfma16<IS_BF16>((v4i){l2[0], l2[1], h2[0], h2[1]}, fb, acc[j]);
                    }
                }
            }
            float x[16];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xe = lowrank ? fmaf(scale, acc[j][e], v[4 * j + e]) : v[4 * j + e];
                    if (row_scale) xe = rsv * xe;
                    x[4 * j + e] = xe;
                }
            if (stats_only) {
                if (run) stat16(x, lo, hi, amax);
                continue;
            }
            if constexpr (MODE != 2) {
                float l = __builtin_inff(), h = -__builtin_inff(), a = 0.0f;
                if (run) stat16(x, l, h, a);
                if (gs >= 32) { l = fminf(l, __shfl_xor(l, 16, 64)); h = fmaxf(h, __shfl_xor(h, 16, 64)); a = fmaxf(a, __shfl_xor(a, 16, 64)); }
                if (gs >= 64) { l = fminf(l, __shfl_xor(l, 32, 64)); h = fmaxf(h, __shfl_xor(h, 32, 64)); a = fmaxf(a, __shfl_xor(a, 32, 64)); }
                if constexpr (MODE == 1) {
                    if (g == 0) { st[0][wave][li] = l; st[1][wave][li] = h; st[2][wave][li] = a; }
                    __syncthreads();
                    const int w1 = wave ^ 1;
                    l = fminf(l, st[0][w1][li]); h = fmaxf(h, st[1][w1][li]); a = fmaxf(a, st[2][w1][li]);
                    if (gs == 256) {
                        const int w2 = wave ^ 2, w3 = wave ^ 3;
                        l = fminf(l, fminf(st[0][w2][li], st[0][w3][li]));
                        h = fmaxf(h, fmaxf(st[1][w2][li], st[1][w3][li]));
                        a = fmaxf(a, fmaxf(st[2][w2][li], st[2][w3][li]));
                    }
                    __syncthreads();  // st is free for the next chunk
                }
                group_scale(asym, l, h, a, o.qmin, o.qmax, s, zp);
                if (run && (k0 % gs) == 0) {
                    const int64_t gi = n * o.G + k0 / gs;
                    o.scale[gi] = s;
                    if (asym) o.zp[gi] = zp;
                }
            }
            if (run) {
                u32* c = codes[tid];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float qv = asym ? (x[j] - zp) / s : x[j] / s;
                    u32 code;
                    SDNQ_ENCODE_QUOTIENT(code, qv, f, is_int, packed, o.qmin, o.qmax);
                    c[j] = code;
                }
                store_codes(o, t, n * p.K + k0, c);
            }
        }
    }
}

struct Span {
    const void* p;
    int64_t bytes;
};
inline bool overlap(const Span& a, const Span& b) {
    if (!a.p || !b.p || a.bytes <= 0 || b.bytes <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + (uintptr_t)b.bytes && b0 < a0 + (uintptr_t)a.bytes;
}

}  // namespace

extern "C" int sdnq_hip_merge_lowrank(const SdnqWeight* w, const SdnqWeight* out, const void* up, const void* down, int dtype, int rank,
                                      float scale, const float* row_scale, float qmin, float qmax, sdnq_stream_t stream) {
    if (!out || !out->weight || !out->scale) return SDNQ_ERR_NULL;
    DeqParams p{};
    const int st = fill_params(w, p);  // NULL, formats, group shape, K % 16, code alignment
    if (st != SDNQ_OK) return st;
    p.svd_up = p.svd_down = nullptr;  // the codes are the residual: the factors stay as they are
    p.rank = 0;
    if ((up == nullptr) != (down == nullptr)) return SDNQ_ERR_NULL;
    if (!up && !row_scale) return SDNQ_ERR_NULL;
    const bool asym = (w->kind == SDNQ_KIND_UINT || w->kind == SDNQ_KIND_UFLOAT);
    if (asym && !out->zero_point) return SDNQ_ERR_NULL;
    if (out->n != w->n || out->k != w->k || out->group_size != w->group_size) return SDNQ_ERR_SHAPE;
    if (out->storage != w->storage || out->kind != w->kind || out->bits != w->bits || out->exponent != w->exponent ||
        out->mantissa != w->mantissa || out->native_float != w->native_float || (out->positions > 1) != (w->positions > 1))
        return SDNQ_ERR_DTYPE;
    // what the fused kernel is not built for: the caller composes sdnq_hip_dequant, a matrix product and the quantizer instead
    if (w->kind == SDNQ_KIND_CODEBOOK || p.P > 1) return SDNQ_ERR_UNSUPPORTED;
    const int gs = p.group_size;
    const bool pow2 = gs == 16 || gs == 32 || gs == 64 || gs == 128 || gs == 256;
    if (!pow2 && gs != p.K) return SDNQ_ERR_UNSUPPORTED;
    if (w->native_float) {
        const bool ok = (w->bits == 8 && ((w->exponent == 4 && w->mantissa == 3) || (w->exponent == 5 && w->mantissa == 2))) ||
                        (w->bits == 16 && ((w->exponent == 5 && w->mantissa == 10) || (w->exponent == 8 && w->mantissa == 7)));
        if (!ok) return SDNQ_ERR_UNSUPPORTED;
    }
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if ((p.N % 8) != 0) return SDNQ_ERR_SHAPE;
    if (up && (rank < 8 || rank > 256 || (rank % 8) != 0)) return SDNQ_ERR_SHAPE;
    if (!(qmax > qmin)) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)up % 16) || ((uintptr_t)down % 16) || ((uintptr_t)row_scale % 4) || ((uintptr_t)out->weight % 16) ||
        ((uintptr_t)out->scale % 4) || ((uintptr_t)out->zero_point % 4))
        return SDNQ_ERR_ALIGN;
    const int64_t gx = (p.N + 15) / 16;
    if (gx > 0x7fffffff) return SDNQ_ERR_SHAPE;
    // no output may overlap an input or another output (a workgroup reads the codes of rows other workgroups have rewritten by then)
    const int64_t nk = p.N * p.K;
    const int64_t code_bytes = w->storage == SDNQ_ST_RAW8 ? nk : w->storage == SDNQ_ST_RAW16 ? 2 * nk : nk / 8 * w->bits;
    const int64_t sc_bytes = p.N * p.G * 4;
    const Span ins[] = {{w->weight, code_bytes}, {w->scale, sc_bytes}, {w->zero_point, sc_bytes}, {up, up ? p.N * rank * 2 : 0},
                        {down, up ? (int64_t)rank * p.K * 2 : 0}, {row_scale, p.N * 4}};
    const Span outs[] = {{out->weight, code_bytes}, {out->scale, sc_bytes}, {asym ? out->zero_point : nullptr, sc_bytes}};
    for (int i = 0; i < 3; ++i) {
        for (const Span& in : ins)
            if (overlap(outs[i], in)) return SDNQ_ERR_SHAPE;
        for (int j = i + 1; j < 3; ++j)
            if (overlap(outs[i], outs[j])) return SDNQ_ERR_SHAPE;
    }
    QuantParams o{};
    o.N = p.N; o.K = p.K; o.group_size = gs; o.G = p.G; o.P = 1; o.SG = p.G;
    o.q = const_cast<void*>(out->weight); o.scale = const_cast<float*>(out->scale);
    o.zp = asym ? const_cast<float*>(out->zero_point) : nullptr;
    o.fmt = p.fmt;
    o.qmin = qmin; o.qmax = qmax;
    const int mode = pow2 ? (gs <= 64 ? 0 : 1) : 2;  // a row-wise weight whose K is one of the five sizes finishes in one sweep too
    PackTable t;
    const int tb = build_table(w->storage, w->bits, t);
    if (tb != SDNQ_OK) return tb;
    // K is shared out over blockIdx.y until about three workgroups per CU of an MI355X are in flight (they fit: 35 KB of LDS, 160 VGPRs);
    // a row-wise weight pays a statistics sweep over all of K per share, so it stops at two per CU.  Measured: profiles/merge_bench.jsonl
    const int64_t chunks = (p.K + MG_KC - 1) / MG_KC;
    const int64_t want = ((mode == 2 ? 512 : 768) + gx - 1) / gx;
    const int64_t shares = want < 1 ? 1 : (want > chunks ? chunks : want);
    const int cpw = (int)((chunks + shares - 1) / shares);
    dim3 grid((unsigned)gx, (unsigned)((chunks + cpw - 1) / cpw)), block(256);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, p, o, t, (const uint16_t*)up, (const uint16_t*)down, rank, scale, row_scale, cpw);
    };
    if (dtype == SDNQ_BF16) {
        if (mode == 0) launch(merge_lowrank_kernel<true, 0>);
        else if (mode == 1) launch(merge_lowrank_kernel<true, 1>);
        else launch(merge_lowrank_kernel<true, 2>);
    } else {
        if (mode == 0) launch(merge_lowrank_kernel<false, 0>);
        else if (mode == 1) launch(merge_lowrank_kernel<false, 1>);
        else launch(merge_lowrank_kernel<false, 2>);
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
