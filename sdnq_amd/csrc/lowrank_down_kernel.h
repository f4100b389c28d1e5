// lowrank_down_kernel of linear_float.hip (its header comment is there) and its dropout form: the activation fragment a lane reads
// from LDS is 8 consecutive k of one row, and one Philox call (philox_dev.h) zeroes its dropped elements in registers before the MFMAs --
// the ring, the stage order and the sums are the plain kernel's: the bits of the plain kernel on a pre-masked x.
// No include guard: the unit includes this file twice, with LR_DROP 0 (the plain kernel, whose text -- and therefore whose code -- is what it
// was before the mask existed) and with LR_DROP 1 (the _dropout kernel: five more arguments and the lines between #if LR_DROP).
#if LR_DROP
#define LR_KERNEL lowrank_down_dropout_kernel
#else
#define LR_KERNEL lowrank_down_kernel
#endif
template <bool IS_BF16, int RT>
__global__ __launch_bounds__(256) void LR_KERNEL(const uint16_t* __restrict__ x, const uint16_t* __restrict__ down,
                                                           uint16_t* __restrict__ t, int64_t M, int64_t K, int64_t ldx, int R
#if LR_DROP
    , u32 thr, u32 seed_lo, u32 seed_hi, u32 off_lo, u32 off_hi
#endif
) {
#if LR_DROP
    SDNQ_KERNARGS_NOW("s"(thr), "s"(seed_lo), "s"(seed_hi), "s"(off_lo), "s"(off_hi));
    const DropArgs drop = {thr, seed_lo, seed_hi, off_lo, off_hi};
#endif
    SDNQ_KERNARGS_NOW("s"(x), "s"(down), "s"(t), "s"(M), "s"(K), "s"(ldx), "s"(R));
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int NS = 4, XS = RT * 16 * 256, STAGE = XS + 32 * 256;  // 12 / 16 KB per stage; 48 / 64 KB ring
    constexpr int NDMA = RT + 2;  // DMAs per wave and stage
    __shared__ __attribute__((aligned(1024))) uint8_t lds[NS * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t m0 = (int64_t)blockIdx.x * (16 * RT);
    const int n_tiles = (R + 31) / 32;
    const int64_t nst = (K + 127) / 128;
    // DMA role of this lane: row 4 * wave + lane / 16 of every activation tile and of each half of the factor tile; physical chunk
    // lane % 16 holds logical chunk (lane % 16) ^ row
    const int drow = wave * 4 + (lane >> 4);
    const int lchunk = (lane & 15) ^ drow;
    // fragment role: row lane & 15, logical chunk 4 * wave + lane / 16 of the stage
    const int frow = lane & 15;
    const int foff = frow * 256 + (((wave * 4 + (lane >> 4)) ^ frow) << 4);
    const uint16_t* sx[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        int64_t gm = m0 + r * 16 + drow;
        if (gm >= M) gm = M - 1;
        sx[r] = x + gm * ldx + lchunk * 8;
    }
    for (int nt = 0; nt < n_tiles; ++nt) {
        const int gn0 = nt * 32 + drow, gn1 = gn0 + 16;
        const uint16_t* sd0 = down + (int64_t)(gn0 < R ? gn0 : 0) * K + lchunk * 8;  // rows past R: valid memory, never stored
        const uint16_t* sd1 = down + (int64_t)(gn1 < R ? gn1 : 0) * K + lchunk * 8;
        auto issue = [&](int64_t st) {  // stages past the end of K are all-zero DMAs: the counted vmcnt stays a constant
            uint8_t* base = lds + (st % NS) * STAGE;
            const int64_t k0 = st * 128;
            const bool ok = k0 + lchunk * 8 < K;
            const uintptr_t z = (uintptr_t)&g_lr_zero16;  // (integer selects: a pointer ternary became three divergent branches)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const uintptr_t px = ok ? (uintptr_t)(sx[r] + k0) : z;
                __builtin_amdgcn_global_load_lds((gptr_t)px, (lptr_t)(base + r * 4096 + wave * 1024), 16, 0, 0);
            }
            const uintptr_t p0 = ok ? (uintptr_t)(sd0 + k0) : z, p1 = ok ? (uintptr_t)(sd1 + k0) : z;
            __builtin_amdgcn_global_load_lds((gptr_t)p0, (lptr_t)(base + XS + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)p1, (lptr_t)(base + XS + 4096 + wave * 1024), 16, 0, 0);
        };
        v4f acc[RT][2];
#pragma unroll
        for (int r = 0; r < RT; ++r) { acc[r][0] = (v4f){0.0f, 0.0f, 0.0f, 0.0f}; acc[r][1] = (v4f){0.0f, 0.0f, 0.0f, 0.0f}; }
#pragma unroll
        for (int s0 = 0; s0 < NS - 1; ++s0) issue(s0);
        for (int64_t st = 0; st < nst; ++st) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * NDMA) : "memory");  // this wave's pieces of stage st have landed
            // ... and everybody's; every wave is also done reading stage st - 1 (its fragments fed MFMAs already), whose slot is
            // refilled next.  Raw s_barrier: __syncthreads() would drain the DMAs in flight (s_waitcnt vmcnt(0)).
            __builtin_amdgcn_s_barrier();
            issue(st + NS - 1);
            const uint8_t* base = lds + (st % NS) * STAGE;
            // (ext-vector loads: an LDS read typed as the HIP uint4 struct makes the compiler drain the LDS-DMAs first, vmcnt(0))
            v4i fx[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) fx[r] = *(const v4i*)(base + r * 4096 + foff);
#if LR_DROP
            {   // the fragment is one 16-byte chunk of x: logical elements m K + k .. + 7 (K % 16 == 0: the chunk index is exact).  A row
                // past M is a clamped load that is never stored; its index comes from the unclamped row and touches no memory
                const int64_t k8 = st * 16 + wave * 4 + (lane >> 4);
#pragma unroll
                for (int r = 0; r < RT; ++r) fx[r] = dropout_chunk(fx[r], (m0 + r * 16 + frow) * (K >> 3) + k8, drop);
            }
#endif
            const v4i f0 = *(const v4i*)(base + XS + foff);
            const v4i f1 = *(const v4i*)(base + XS + 4096 + foff);
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                if constexpr (IS_BF16) {
                    acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, f0), __builtin_bit_cast(v8bf, fx[r]), acc[r][0], 0, 0, 0);
                    acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, f1), __builtin_bit_cast(v8bf, fx[r]), acc[r][1], 0, 0, 0);
                } else {
                    acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, f0), __builtin_bit_cast(v8h, fx[r]), acc[r][0], 0, 0, 0);
                    acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, f1), __builtin_bit_cast(v8h, fx[r]), acc[r][1], 0, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing zero DMAs target the ring the partial sums reuse
        __syncthreads();
        float* part = (float*)lds;  // [4 waves][RT row tiles][2 rank halves][4 regs][64 lanes]
        constexpr int WSTRIDE = RT * 2 * 4 * 64;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) part[wave * WSTRIDE + ((r * 2 + h) * 4 + e) * 64 + lane] = acc[r][h][e];
        __syncthreads();
        // accumulator layout: lane l of (row tile r, rank half h) holds n = 16 h + 4 (l >> 4) + e, m = 16 r + (l & 15).  Consecutive
        // threads take consecutive n of one row (64-byte runs of t)
#pragma unroll
        for (int o = tid; o < RT * 512; o += 256) {
            const int n = o & 31, m = o >> 5;
            const int r = m >> 4, ml = m & 15, h = n >> 4, q = n & 15, l = (q >> 2) * 16 + ml, e = q & 3;
            const int idx = ((r * 2 + h) * 4 + e) * 64 + l;
            const float sum = (part[idx] + part[WSTRIDE + idx]) + (part[2 * WSTRIDE + idx] + part[3 * WSTRIDE + idx]);
            const int gn = nt * 32 + n;
            if (m0 + m < M && gn < R) t[(m0 + m) * R + gn] = IS_BF16 ? f32_to_bf16_bits(sum) : f32_to_f16_bits(sum);
        }
        __syncthreads();  // partial sums consumed before the next n-tile's DMAs overwrite them
    }
}
#undef LR_KERNEL
