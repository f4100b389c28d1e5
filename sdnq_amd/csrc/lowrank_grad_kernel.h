// lowrank_grad_kernel of lowrank_train.hip (its header comment is there) and its dropout form: the mask falls on `a` as it is staged
// -- one Philox call (philox_dev.h) per 16-byte chunk of `fetch`, before `stash`; everything behind it is the plain kernel.
// No include guard: the unit includes this file twice, with LR_DROP 0 (the plain kernel, whose text -- and therefore whose code -- is what it
// was before the mask existed) and with LR_DROP 1 (the _dropout kernel: five more arguments and the lines between #if LR_DROP).
#if LR_DROP
#define LR_KERNEL lowrank_grad_dropout_kernel
#else
#define LR_KERNEL lowrank_grad_kernel
#endif
// NRT: rank tiles of 16 (rank <= 16 NRT).  grid (column tiles of a, slabs).  `direct`: one slab -- scale, round and store out; otherwise
// the float32 partial goes to part [slab][P][R].
template <bool IS_BF16, int NRT>
__global__ __launch_bounds__(256) void LR_KERNEL(const uint16_t* __restrict__ a, int64_t lda, const uint16_t* __restrict__ b,
                                                           int64_t M, int64_t P, int R, float scale, int out_t, void* __restrict__ out,
                                                           int out_dtype, float* __restrict__ part, int direct
#if LR_DROP
    , u32 thr, u32 seed_lo, u32 seed_hi, u32 off_lo, u32 off_hi
#endif
) {
#if LR_DROP
    SDNQ_KERNARGS_NOW("s"(thr), "s"(seed_lo), "s"(seed_hi), "s"(off_lo), "s"(off_hi));
    const DropArgs drop = {thr, seed_lo, seed_hi, off_lo, off_hi};
#endif
    SDNQ_KERNARGS_NOW("s"(a), "s"(lda), "s"(b), "s"(M), "s"(P), "s"(R), "s"(scale), "s"(out_t), "s"(out), "s"(out_dtype), "s"(part), "s"(direct));
    constexpr int ROWS = 64, AB = 128, BB = NRT * 32;            // rows per stage; bytes per LDS row of a / b
    constexpr int BCH = NRT * 2;                                  // 16-byte chunks per row of b
    constexpr int NB = (ROWS * BCH + 255) / 256;                  // chunks of b per thread and stage
    __shared__ __attribute__((aligned(16))) uint8_t img_a[ROWS * AB];
    __shared__ __attribute__((aligned(16))) uint8_t img_b[ROWS * BB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    const int64_t i_begin = (int64_t)blockIdx.y * LRG_SLAB;
    const int64_t i_end = i_begin + LRG_SLAB < M ? i_begin + LRG_SLAB : M;
    const v4i zero = {0, 0, 0, 0};
    // staging roles: a -- chunks tid and tid + 256 of 512 (row = chunk / 8, 8 columns each); b -- chunks tid + 256 x of ROWS * BCH
    v4i ra[2], rb[NB];
    auto fetch = [&](int64_t i0) {
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int ch = tid + 256 * x, row = ch >> 3, col = (ch & 7) * 8;
            const int64_t i = i0 + row, j = j0 + col;
            ra[x] = (i < i_end && j < P) ? *(const v4i*)(a + i * lda + j) : zero;  // P % 8 == 0
#if LR_DROP
            if (i < i_end && j < P) ra[x] = dropout_chunk(ra[x], i * (P >> 3) + (j >> 3), drop);  // logical elements i P + j .. + 7 of a
#endif
        }
#pragma unroll
        for (int x = 0; x < NB; ++x) {
            const int ch = tid + 256 * x, row = ch / BCH, col = (ch % BCH) * 8;
            const int64_t i = i0 + row;
            rb[x] = (ch < ROWS * BCH && i < i_end && col < R) ? *(const v4i*)(b + i * R + col) : zero;  // rank % 8 == 0
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int ch = tid + 256 * x, row = ch >> 3, c8 = ch & 7;
            *(v4i*)(img_a + row * AB + (((c8 >> 1) ^ lrg_swz<4>(row)) << 5) + ((c8 & 1) << 4)) = ra[x];
        }
#pragma unroll
        for (int x = 0; x < NB; ++x) {
            const int ch = tid + 256 * x, row = ch / BCH, c8 = ch % BCH;
            if (ch < ROWS * BCH) *(v4i*)(img_b + row * BB + (((c8 >> 1) ^ lrg_swz<NRT>(row)) << 5) + ((c8 & 1) << 4)) = rb[x];
        }
    };
    v4f acc[NRT];
#pragma unroll
    for (int r = 0; r < NRT; ++r) acc[r] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    fetch(i_begin);
    for (int64_t i0 = i_begin; i0 < i_end; i0 += ROWS) {
        __syncthreads();  // the previous stage's fragments are read
        stash();
        __syncthreads();
        if (i0 + ROWS < i_end) fetch(i0 + ROWS);  // (block-uniform) in flight under the MFMAs
#pragma unroll
        for (int s = 0; s < ROWS; s += 32) {
            const v4i fa = lrg_frag<4>(img_a, s, wave, lane);
#pragma unroll
            for (int r = 0; r < NRT; ++r) acc[r] = mfma16<IS_BF16>(fa, lrg_frag<NRT>(img_b, s, r, lane), acc[r]);
        }
    }
    // accumulator e of rank tile r: column j = j0 + 16 wave + 4 (lane / 16) + e of a, rank 16 r + lane % 16
    const int64_t jb = j0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < NRT; ++r) {
        const int rr = 16 * r + (lane & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = jb + e;
            if (j < P && rr < R) {
                if (direct) st_rt(out, out_t ? (int64_t)rr * P + j : j * R + rr, scale * acc[r][e], out_dtype);
                else part[((int64_t)blockIdx.y * P + j) * R + rr] = acc[r][e];
            }
        }
    }
}
#undef LR_KERNEL
