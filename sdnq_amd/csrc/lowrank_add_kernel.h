// lowrank_add_kernel of lowrank_train.hip (its header comment is there) and its dropout form: the epilogue's 8 columns of a lane
// are one 16-byte chunk of y, and one Philox call (philox_dev.h) says which of them take the adapter's term.
// No include guard: the unit includes this file once per form, with LR_DROP 0 (the plain kernel, whose text -- and therefore whose code -- is
// what it was before the mask existed), with LR_DROP 1 (the _dropout kernel: five more arguments and the lines between #if LR_DROP) and
// with LR_DORA 1 (sdnq_hip_lowrank_add_dora: the magnitude column scale c [N] and the bias as two more arguments, and its own epilogue).
#if LR_DORA
#define LR_KERNEL lowrank_add_dora_kernel
#elif LR_DROP
#define LR_KERNEL lowrank_add_dropout_kernel
#else
#define LR_KERNEL lowrank_add_kernel
#endif
// RT: 16-row tiles per wave (a workgroup owns 64 RT rows): every fragment of up feeds RT MFMAs
template <int T_ID, int RT>
__global__ __launch_bounds__(256) void LR_KERNEL(const uint16_t* __restrict__ t, const uint16_t* __restrict__ up,
                                                          uint16_t* __restrict__ y, int64_t M, int64_t N, int64_t ldy, int R, float scale
#if LR_DROP
    , u32 thr, u32 seed_lo, u32 seed_hi, u32 off_lo, u32 off_hi
#endif
#if LR_DORA
    , const float* __restrict__ cvec, const uint16_t* __restrict__ bias
#endif
) {
#if LR_DORA
    SDNQ_KERNARGS_NOW("s"(cvec), "s"(bias));
#endif
#if LR_DROP
    SDNQ_KERNARGS_NOW("s"(thr), "s"(seed_lo), "s"(seed_hi), "s"(off_lo), "s"(off_hi));
    const DropArgs drop = {thr, seed_lo, seed_hi, off_lo, off_hi};
#endif
    SDNQ_KERNARGS_NOW("s"(t), "s"(up), "s"(y), "s"(M), "s"(N), "s"(ldy), "s"(R), "s"(scale));
    constexpr bool IS_BF16 = T_ID == SDNQ_BF16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    // this lane's rows of y (B operand: column li of the MFMA), one per row tile
    const int64_t m0 = ((int64_t)blockIdx.y * 4 + wave) * (16 * RT) + li;
    const int64_t n0 = (int64_t)blockIdx.x * 128;
    // A operand: MFMA row li of tile (c, h) is column n0 + 32 c + 8 (li / 4) + 4 h + li % 4 of y
    const int64_t na = n0 + 8 * (li >> 2) + (li & 3);
    v4f acc[RT][4][2];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c][0] = acc[r][c][1] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    const v4i zero = {0, 0, 0, 0};
    for (int k0 = 0; k0 < R; k0 += 32) {
        const int kc = k0 + 8 * g;      // this lane's rank chunk of the step
        const bool k_ok = kc < R;       // rank % 8 == 0: a chunk is inside the row or past it
        v4i fb[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int64_t m = m0 + 16 * r;
            fb[r] = (k_ok && m < M) ? *(const v4i*)(t + m * R + kc) : zero;
        }
        v4i fa[4][2];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t n = na + 32 * c + 4 * h;
                fa[c][h] = (k_ok && n < N) ? *(const v4i*)(up + n * R + kc) : zero;
            }
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h) acc[r][c][h] = mfma16<IS_BF16>(fa[c][h], fb[r], acc[r][c][h]);
    }
    // lane (row m, g): accumulators acc[r][c][h][e] = column n0 + 32 c + 8 g + 4 h + e
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int64_t m = m0 + 16 * r;
        if (m >= M) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t n = n0 + 32 * c + 8 * g;
            if (n < N) {  // N % 8 == 0: the 8 columns are inside the row or past it
                uint4* p = (uint4*)(y + m * ldy + n);
                float f[8];
                Vec16<T_ID>::unpack(*p, f);
#if LR_DROP
                // the 8 columns are logical elements m N + n .. + 7 of y (N % 8 == 0: the chunk index is exact).  A dropped element's sum
                // becomes +0.0, and the plain epilogue below -- the same text -- stores an element with a zero sum back as it was read
                {
                    const u32 keep = dropout_keep8(m * (N >> 3) + (n >> 3), drop);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[r][c][0][e] = ((keep >> e) & 1u) ? acc[r][c][0][e] : 0.0f;
                        acc[r][c][1][e] = ((keep >> (4 + e)) & 1u) ? acc[r][c][1][e] : 0.0f;
                    }
                }
#endif
#if LR_DORA
                // DoRA: y = c (u + scale acc) + b from the stored z = u + b, as round(fmaf(c scale, acc, fmaf(c - 1, z - b, z))).  With
                // c == 1 the inner term IS z (kept as read, so that a -0.0 or an infinity is not touched by 0 * (z - b)) and the store is the
                // plain kernel's below, its exactly-zero-sum rule included: a fresh adapter leaves every bit of y alone
                {
                    float cj[8], bj[8];
                    Vec16<SDNQ_F32>::unpack(*(const uint4*)(cvec + n), cj);
                    Vec16<SDNQ_F32>::unpack(*(const uint4*)(cvec + n + 4), cj + 4);
                    if (bias) Vec16<T_ID>::unpack(*(const uint4*)(bias + n), bj);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (!bias) bj[e] = 0.0f;
                        const float a = acc[r][c][e >> 2][e & 3], cm1 = cj[e] - 1.0f, cs = cj[e] * scale;
                        const float inner = cm1 == 0.0f ? f[e] : fmaf(cm1, f[e] - bj[e], f[e]);
                        f[e] = a == 0.0f ? inner : fmaf(cs, a, inner);
                    }
                }
#else
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // a sum that is exactly zero leaves the element as it is: fmaf(scale, +0, -0.0) is +0.0
                    const float a0 = acc[r][c][0][e], a1 = acc[r][c][1][e];
                    f[e] = a0 == 0.0f ? f[e] : fmaf(scale, a0, f[e]);
                    f[4 + e] = a1 == 0.0f ? f[4 + e] : fmaf(scale, a1, f[4 + e]);
                }
#endif
                *p = Vec16<T_ID>::pack(f);
            }
        }
    }
}
#undef LR_KERNEL
