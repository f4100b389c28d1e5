// Load-time weight quantizer for gfx950: float [N][K] weight -> codes in the reference's storage
// format + f32 group scales (+ zero points).
//
//   pass 1  quant_stats_kernel : per (row, group) min / max / amax -> scale, zero_point   (quant_utils.py:10-24)
//   pass 2  quant_pack_kernel  : q = w / s  or  (w - zp) / s ; ints: round-half-even, clamp; floats: nan_to_num, clamp,
//                                convert (quant_utils.py:28-56) ; then the reference's packing:
//                                signed ints stored as value - min (packed_int/__init__.py:77-80), bit-interleaved group
//                                codecs (packed_int/pack.py), eXmY float encoder with its own rounding rule
//                                (packed_float.py:27-82).
//
// The bit placement of every packed format is NOT written out a second time: the host derives it by probing the decoders
// of unpack_dev.h one word bit at a time (each word bit feeds exactly one element bit), so packer and unpacker cannot
// disagree; the goldens captured from the reference pin both.
//
// HBM-bound, run once per layer: N*K*(src bytes) read twice (2nd pass mostly L2-hot per row block) + N*K*bits/8 written.
// PackTable, the per-element encode step, the float encoders and the packers are in quant_dev.h, shared with merge.hip.
#include "quant_dev.h"

namespace {

template <int LANES>
__device__ __forceinline__ float sub_max(float v) {
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int LANES>
__device__ __forceinline__ float sub_min(float v) {
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// LANES consecutive lanes own one (row, group)
template <int SRC_T, int LANES>
__global__ __launch_bounds__(256) void quant_stats_kernel(const QuantParams p) {
    const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LANES;
    const int l = threadIdx.x % LANES;
    const bool live = gid < p.N * p.SG;
    const int64_t n = live ? gid / p.SG : 0;
    const int sg = live ? (int)(gid % p.SG) : 0;
    // Linear: group g = sg, elements contiguous.  Conv (P > 1): sg = (channel group, position); the group's elements are the
    // group's channels at that kernel position: k = (cg * group_size + j) * P + pos
    const int64_t base = n * p.ld + (int64_t)(sg / p.P) * p.group_size * p.P + (sg % p.P);
    float lo = __builtin_inff(), hi = -__builtin_inff(), amax = 0.0f;
    if (live) {
        for (int j = l; j < p.group_size; j += LANES) {
            const float v = FT<SRC_T>::load(p.src, base + (int64_t)j * p.P);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
            amax = fmaxf(amax, fabsf(v));
        }
    }
    lo = sub_min<LANES>(lo);
    hi = sub_max<LANES>(hi);
    amax = sub_max<LANES>(amax);
    if (!live || l != 0) return;
    const bool asym = (p.fmt.kind == SDNQ_KIND_UINT || p.fmt.kind == SDNQ_KIND_UFLOAT);
    if (asym) {
        const float s = (hi - lo) / (p.qmax - p.qmin);
        p.scale[gid] = s;
        p.zp[gid] = (p.qmin == 0.0f) ? lo : lo - s * p.qmin;
    } else {
        p.scale[gid] = amax / p.qmax;
    }
}

// one thread = 16 consecutive elements of one row (K % 16 == 0), codes staged in LDS for table-driven bit placement
template <int SRC_T>
__global__ __launch_bounds__(256) void quant_pack_kernel(const QuantParams p, const PackTable t) {
    __shared__ u32 codes[256][17];
    const int64_t units_per_row = p.K / 16;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= p.N * units_per_row) return;
    const int64_t n = u / units_per_row, k0 = (u % units_per_row) * 16;
    const WeightFmt f = p.fmt;
    const bool asym = (f.kind == SDNQ_KIND_UINT || f.kind == SDNQ_KIND_UFLOAT);
    const bool is_int = (f.kind == SDNQ_KIND_INT || f.kind == SDNQ_KIND_UINT);
    const bool packed = (f.storage == SDNQ_ST_PACKED_U8 || f.storage == SDNQ_ST_PACKED_I16);
    u32* c = codes[threadIdx.x];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float w = FT<SRC_T>::load(p.src, n * p.ld + k0 + j);
        const int kk = (int)(k0 + j), cc = kk / p.P;
        const int64_t gi = n * p.SG + (p.P > 1 ? (cc / p.group_size) * p.P + (kk - cc * p.P) : kk / p.group_size);
        const float s = p.scale[gi];
        float q = asym ? (w - p.zp[gi]) / s : w / s;
        u32 code;
        SDNQ_ENCODE_QUOTIENT(code, q, f, is_int, packed, p.qmin, p.qmax);
        c[j] = code;
    }
    store_codes(p, t, n * p.K + k0, c);
}

// ---- codebook quantizer (quantize_weight_codebook, quant_utils.py:59-120) ------------------------------------------------------
// One wave per reduction slice; the slice's values live in LDS.  Every step of the reference is restated with its own rounding:
// the initial levels are one fma, the midpoints (a + b) * 0.5, the assignment a search that sends a value on a midpoint to the lower
// level, and each level's new value the sum of its members IN ELEMENT ORDER (the reference's CPU scatter_add_) divided by their
// count.  A tree reduction would round differently, and 24 rounds turn one ulp into different codes, so the members are first
// grouped by level with a stable counting partition (integer prefix sums, ballots within a 64-element chunk -- exact), after which
// one lane per level adds its members in order: linear work per round instead of a scan of the whole slice per level.
constexpr int CB_MAX_LEVELS = 256;
constexpr int CB_MAX_SLICE = 16384;
__host__ __device__ constexpr size_t cb_lds_bytes(int slice) { return (size_t)4 * CB_MAX_LEVELS * 4 + (size_t)slice * 9; }

struct CbParams {
    const void* src;
    int64_t ld, N;
    int group_size, G, P, L, steps;
    float* levels;  // [N][G][L][P]
};

// index of the first midpoint >= x among mid[0 .. L-2] (torch.searchsorted, side="left"): the number of midpoints below x
__device__ __forceinline__ int cb_search(const float* mid, int L, float x) {
    int lo = 0, hi = L - 1;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (mid[m] < x) lo = m + 1;
        else hi = m;
    }
    return lo;
}

template <int SRC_T>
__global__ __launch_bounds__(64) void codebook_kernel(const CbParams p) {
    extern __shared__ float cb_sm[];
    float* lev = cb_sm;                                        // [L] levels
    float* mid = cb_sm + CB_MAX_LEVELS;                        // [L - 1] midpoints
    int* cnt = (int*)(cb_sm + 2 * CB_MAX_LEVELS);              // [L] members per level
    int* run = (int*)(cb_sm + 3 * CB_MAX_LEVELS);              // [L] next free slot of each level in `perm`
    float* vals = cb_sm + 4 * CB_MAX_LEVELS;                   // [S] the slice in element order
    float* perm = vals + p.group_size;                         // [S] the slice grouped by level, element order within a level
    uint8_t* asg = (uint8_t*)(perm + p.group_size);            // [S] level of each element
    const int lane = threadIdx.x, S = p.group_size, L = p.L;
    const int64_t sid = blockIdx.x;
    const int64_t n = sid / ((int64_t)p.G * p.P);
    const int r = (int)(sid - n * p.G * p.P), g = r / p.P, pos = r - g * p.P;
    const int64_t base = n * p.ld + (int64_t)g * S * p.P + pos;  // element j of the slice: base + j * P
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int j = lane; j < S; j += 64) {
        const float v = FT<SRC_T>::load(p.src, base + (int64_t)j * p.P);
        vals[j] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    const float step = (hi - lo) / (float)(L - 1);
    for (int l = lane; l < L; l += 64) lev[l] = fmaf((float)l, step, lo);  // torch.addcmul: one rounding
    __syncthreads();
    for (int it = 0;; ++it) {
        // sort: each level's rank is the number of levels below it (ties in index order); ranks < L, so every write stays in lev[]
        float x[CB_MAX_LEVELS / 64];
        int rk[CB_MAX_LEVELS / 64];
#pragma unroll
        for (int q = 0; q < CB_MAX_LEVELS / 64; ++q) {
            const int l = lane + 64 * q;
            rk[q] = -1;
            if (l < L) {
                x[q] = lev[l];
                int c = 0;
                for (int j = 0; j < L; ++j) {
                    const float y = lev[j];
                    c += (y < x[q]) || (y == x[q] && j < l);
                }
                rk[q] = c;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CB_MAX_LEVELS / 64; ++q)
            if (rk[q] >= 0) lev[rk[q]] = x[q];
        __syncthreads();
        if (it == p.steps) break;
        for (int l = lane; l < L - 1; l += 64) mid[l] = (lev[l] + lev[l + 1]) * 0.5f;
        for (int l = lane; l < L; l += 64) cnt[l] = 0;
        __syncthreads();
        for (int j = lane; j < S; j += 64) {
            const int a = cb_search(mid, L, vals[j]);
            asg[j] = (uint8_t)a;
            atomicAdd(&cnt[a], 1);
        }
        __syncthreads();
        if (lane == 0) {
            int acc = 0;
            for (int l = 0; l < L; ++l) { run[l] = acc; acc += cnt[l]; }
        }
        __syncthreads();
        // stable partition, 64 elements at a time: a lane's slot is its level's next free slot + the number of lower lanes in the
        // chunk with the same level (peers found by one ballot per code bit)
        for (int c0 = 0; c0 < S; c0 += 64) {
            const int j = c0 + lane;
            const bool live = j < S;
            const int a = live ? asg[j] : 0;
            uint64_t peers = __ballot(live);
            for (int b = 0; b < 8; ++b) {
                const uint64_t m = __ballot(live && ((a >> b) & 1));
                peers &= ((a >> b) & 1) ? m : ~m;
            }
            const int rank = __popcll(peers & ((1ull << lane) - 1ull));
            const int total = __popcll(peers);
            const int slot = live ? run[a] + rank : 0;
            __syncthreads();
            if (live) {
                perm[slot] = vals[j];
                if (rank == total - 1) run[a] = slot + 1;
            }
            __syncthreads();
        }
        // levels with members: their sum in element order / count; empty levels keep their value
        for (int l = lane; l < L; l += 64) {
            const int c = cnt[l];
            if (c > 0) {
                const int start = run[l] - c;
                float sum = 0.0f;
                for (int i = 0; i < c; ++i) sum += perm[start + i];
                lev[l] = sum / (float)c;
            }
        }
        __syncthreads();
    }
    float* out = p.levels + ((n * p.G + g) * (int64_t)L) * p.P + pos;
    for (int l = lane; l < L; l += 64) out[(int64_t)l * p.P] = lev[l];
}

// the final assignment of every element against its slice's sorted levels (the same search as codebook_kernel), packed like
// quant_pack_kernel's codes
template <int SRC_T>
__global__ __launch_bounds__(256) void codebook_pack_kernel(const QuantParams p, const PackTable t, const CbParams cb) {
    const int64_t units_per_row = p.K / 16;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= p.N * units_per_row) return;
    const int64_t n = u / units_per_row, k0 = (u % units_per_row) * 16;
    const int L = cb.L;
    u32 c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float w = FT<SRC_T>::load(p.src, n * p.ld + k0 + j);
        const int kk = (int)(k0 + j), cc = kk / p.P, pos = kk - cc * p.P;
        const float* lv = cb.levels + ((n * p.G + cc / p.group_size) * (int64_t)L) * p.P + pos;  // level i at lv[i * P]
        int lo = 0, hi = L - 1;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if ((lv[(int64_t)m * p.P] + lv[(int64_t)(m + 1) * p.P]) * 0.5f < w) lo = m + 1;
            else hi = m;
        }
        c[j] = (u32)lo;
    }
    store_codes(p, t, n * p.K + k0, c);
}

template <int SRC_T>
int launch_codebook(const QuantParams& p, const PackTable& t, const CbParams& cb, hipStream_t s) {
    const size_t lds = cb_lds_bytes(cb.group_size);
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)codebook_kernel<SRC_T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)cb_lds_bytes(CB_MAX_SLICE)) != hipSuccess)
        return SDNQ_ERR_LAUNCH;
    hipLaunchKernelGGL((codebook_kernel<SRC_T>), dim3((unsigned)(p.N * cb.G * cb.P)), dim3(64), lds, s, cb);
    SDNQ_CHECK_LAUNCH();
    const int64_t units = p.N * (p.K / 16);
    hipLaunchKernelGGL((codebook_pack_kernel<SRC_T>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, p, t, cb);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

template <int SRC_T>
int launch(const QuantParams& p, const PackTable& t, hipStream_t s) {
    const int64_t groups = p.N * p.SG;
    const int gs = p.group_size;
#define STATS(L)                                                                                              \
    hipLaunchKernelGGL((quant_stats_kernel<SRC_T, L>), dim3((unsigned)((groups * L + 255) / 256)), dim3(256), 0, s, p)
    if (gs >= 512) STATS(64);
    else if (gs >= 128) STATS(16);
    else if (gs >= 32) STATS(4);
    else STATS(1);
#undef STATS
    SDNQ_CHECK_LAUNCH();
    const int64_t units = p.N * (p.K / 16);
    hipLaunchKernelGGL((quant_pack_kernel<SRC_T>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, p, t);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

}  // namespace

extern "C" int sdnq_hip_quantize_weight(const void* src, int src_dtype, int64_t ld_src, const SdnqWeight* w, float qmin,
                                        float qmax, sdnq_stream_t stream) {
    if (!src || !w || !w->weight || !w->scale) return SDNQ_ERR_NULL;
    if (src_dtype < 0 || src_dtype > 2) return SDNQ_ERR_DTYPE;
    const int pos = w->positions > 1 ? w->positions : 1;
    if (w->n <= 0 || w->k <= 0 || w->group_size <= 0 || (w->k % pos) != 0 || ((w->k / pos) % w->group_size) != 0 || (w->k % 16) != 0) return SDNQ_ERR_SHAPE;
    if (w->storage < 0 || w->storage > 3 || w->kind < 0 || w->kind > 3 || w->bits < 1 || w->bits > 16) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_PACKED_U8 && w->bits > 7) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_PACKED_I16 && (w->bits < 9 || w->bits > 15)) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_RAW8 && w->bits != 8) return SDNQ_ERR_DTYPE;
    if (w->storage == SDNQ_ST_RAW16 && w->bits != 16) return SDNQ_ERR_DTYPE;
    const bool asym = (w->kind == SDNQ_KIND_UINT || w->kind == SDNQ_KIND_UFLOAT);
    const bool is_float = (w->kind == SDNQ_KIND_FLOAT || w->kind == SDNQ_KIND_UFLOAT);
    if (asym && !w->zero_point) return SDNQ_ERR_NULL;
    if (is_float && !w->native_float) {
        const int sign = (w->kind == SDNQ_KIND_FLOAT) ? 1 : 0;
        if (w->exponent < 1 || w->exponent > 7 || w->mantissa < 0 || sign + w->exponent + w->mantissa != w->bits) return SDNQ_ERR_DTYPE;
    }
    if (is_float && w->native_float) {
        const bool ok = (w->bits == 8 && ((w->exponent == 4 && w->mantissa == 3) || (w->exponent == 5 && w->mantissa == 2))) ||
                        (w->bits == 16 && ((w->exponent == 5 && w->mantissa == 10) || (w->exponent == 8 && w->mantissa == 7)));
        if (!ok) return SDNQ_ERR_UNSUPPORTED;
    }
    if (!(qmax > qmin)) return SDNQ_ERR_SHAPE;
    if ((uintptr_t)w->weight % 16) return SDNQ_ERR_ALIGN;
    QuantParams p{};
    p.src = src; p.ld = ld_src; p.N = w->n; p.K = w->k; p.group_size = w->group_size; p.G = (w->k / pos) / w->group_size; p.P = pos; p.SG = p.G * pos;
    p.q = const_cast<void*>(w->weight); p.scale = const_cast<float*>(w->scale); p.zp = const_cast<float*>(w->zero_point);
    p.fmt = WeightFmt{w->storage, w->kind, w->bits, w->exponent, w->mantissa, w->native_float};
    p.qmin = qmin; p.qmax = qmax;
    PackTable t;
    int st = build_table(w->storage, w->bits, t);
    if (st != SDNQ_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype == SDNQ_F32) return launch<SDNQ_F32>(p, t, s);
    if (src_dtype == SDNQ_BF16) return launch<SDNQ_BF16>(p, t, s);
    return launch<SDNQ_F16>(p, t, s);
}

extern "C" int sdnq_hip_quantize_codebook(const void* src, int src_dtype, int64_t ld_src, const SdnqWeight* w, int steps,
                                          sdnq_stream_t stream) {
    if (!src || !w || !w->weight || !w->scale) return SDNQ_ERR_NULL;
    if (src_dtype < 0 || src_dtype > 2) return SDNQ_ERR_DTYPE;
    if (w->kind != SDNQ_KIND_CODEBOOK || w->bits < 1 || w->bits > 8 || w->native_float) return SDNQ_ERR_DTYPE;
    if (w->storage != (w->bits == 8 ? SDNQ_ST_RAW8 : SDNQ_ST_PACKED_U8)) return SDNQ_ERR_DTYPE;
    if (w->zero_point) return SDNQ_ERR_UNSUPPORTED;
    const int pos = w->positions > 1 ? w->positions : 1;
    if (w->n <= 0 || w->k <= 0 || w->group_size <= 0 || (w->k % pos) != 0 || ((w->k / pos) % w->group_size) != 0 || (w->k % 16) != 0) return SDNQ_ERR_SHAPE;
    if (ld_src < w->k) return SDNQ_ERR_SHAPE;
    if (w->group_size > CB_MAX_SLICE || steps < 0 || steps > 1024) return SDNQ_ERR_UNSUPPORTED;
    if ((uintptr_t)w->weight % 16) return SDNQ_ERR_ALIGN;
    QuantParams p{};
    p.src = src; p.ld = ld_src; p.N = w->n; p.K = w->k; p.group_size = w->group_size; p.G = (w->k / pos) / w->group_size; p.P = pos;
    p.SG = p.G * pos;
    p.q = const_cast<void*>(w->weight);
    p.fmt = WeightFmt{w->storage, w->kind, w->bits, 0, 0, 0};
    if (p.N * p.G * pos > 0x7fffffffLL) return SDNQ_ERR_SHAPE;
    CbParams cb{};
    cb.src = src; cb.ld = ld_src; cb.N = w->n; cb.group_size = w->group_size; cb.G = p.G; cb.P = pos; cb.L = 1 << w->bits; cb.steps = steps;
    cb.levels = const_cast<float*>(w->scale);
    PackTable t;
    int st = build_table(w->storage, w->bits, t);
    if (st != SDNQ_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype == SDNQ_F32) return launch_codebook<SDNQ_F32>(p, t, cb, s);
    if (src_dtype == SDNQ_BF16) return launch_codebook<SDNQ_BF16>(p, t, cb, s);
    return launch_codebook<SDNQ_F16>(p, t, cb, s);
}
