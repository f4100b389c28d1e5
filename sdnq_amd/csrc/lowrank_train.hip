// Trainable low-rank adapters (LoRA) on frozen quantized Linear layers: the two products of the adapter branch that are no plain
// [M][K] x [N][K]^T (those run on sdnq_hip_lowrank_down and the float GEMM).  No reference interface: the reference has no adapters;
// these replace what a user assembles from torch ops around the quantized layer.
//
//   sdnq_hip_lowrank_add   y += scale * t . up^T in place, the up-projection of the forward and the down^T term of grad_input:
//       y[i][j] = round_dtype( fmaf(scale, sum_r t[i][r] * up[j][r], y[i][j]) ), ONE rounding per element, one read and one write of y
//       (a sum that is exactly zero leaves the element's bits alone, a -0.0 included: up == 0 changes nothing).
//       A workgroup (4 waves) owns 64 RT rows x 128 columns, wave w RT tiles of 16 rows (RT = 2 once the launch still has two workgroups
//       per CU: a fragment of up then feeds two MFMAs).  The sum runs on v_mfma_f32_16x16x32 as
//       C^T = up . t^T: A = 16 rows of up, B = 16 rows of t, so that a lane's four accumulators are four COLUMNS of one row of y; which
//       16 rows of up an MFMA takes is free, and tile 2c takes columns 8 g + e, tile 2c + 1 columns 8 g + 4 + e (g = 0..3, e = 0..3) of
//       the 32-column block c -- a lane (row lane % 16, g = lane / 16) then holds the 8 consecutive columns 32 c + 8 g .. + 7: one 16-byte
//       load and store of y per block.  Both operands are read straight from global memory in fragment form (16 bytes per lane: lane
//       l = row l % 16, rank chunk l / 16 of the 32-rank step); they are [M][rank] and [N][rank], a few KB per workgroup, and stay in
//       L1 / L2.  A rank chunk at or past `rank` is a zero fragment in registers: nothing is read past a row.  No LDS, no workspace.
//
//   sdnq_hip_lowrank_grad  out = scale * a^T . b, the factor gradients (grad_up = dY^T . t, grad_down^T = x^T . g_t): a product that
//       reduces over the ROWS, the slow axis of both operands in memory.  M is cut into slabs of LRG_SLAB rows -- a constant of this
//       file, not of the device or the grid -- and a workgroup computes the float32 partial of one (64-column tile of a, slab):
//       stages of 64 rows of both operands go to LDS as they lie in memory (16-byte chunks, rows past the slab / columns past P / rank
//       columns past `rank` as zeros), and the MFMA operands, which need 8 consecutive ROWS of one column per lane, come out of it by
//       ds_read_b64_tr_b16 (a 16-lane group reads 4 rows x 16 columns transposed).  Wave w owns columns 16 w .. 16 w + 15 of the tile
//       and every rank tile (NRT x 16 columns: 4 NRT accumulators).  One slab: the workgroup scales, rounds and stores out itself.
//       More: the partials go to workspace [slab][P][rank] and a second launch adds them in ascending slab order, scales and rounds --
//       no atomics, the same bits on every call.
//       LDS images, rows of 128 bytes (a) and 32 NRT bytes (b); the 32-byte column pair cp of row i lies at pair cp ^ swz(i):
//         transposed reads (banks = dword % 64, conflicts inside a 32-lane half): a half reads rows {8 g + q} and {8 (g + 1) + q},
//         q = 0..3, of one column pair, 32 bytes each.  128-byte rows: rows two apart share their banks, swz = (i / 2) % 2 + 2 * ((i / 8)
//         % 2) sends the four of them to the four pairs: conflict-free.  256- and 512-byte rows: every row starts on bank 0, swz = i % 4 +
//         4 * ((i / 8) % 2) gives the 8 rows 8 different pairs: conflict-free.  64-byte rows: rows 8 apart collide, swz = (i / 8) % 2.
//         32-byte rows (rank <= 16): one pair per row, the two blocks of a half are 256 bytes apart: 2-way, left as it is.
//       The bank arithmetic is worked out by hand from the guide's tables; no counter run has confirmed it.  The global loads of the
//       next stage are issued before the MFMAs of the current one; otherwise untuned.
#include "lowrank_dev.h"  // mfma16, lrg_swz, lrg_frag, lowrank_grad_sum_kernel: shared with conv_lowrank.hip

namespace {

constexpr int LRG_SLAB = 256;  // rows of M per partial sum of sdnq_hip_lowrank_grad (tests/lora_util.py restates it)

// ---- y += scale * t . up^T ------------------------------------------------------------------------------------------------------------
// RT: 16-row tiles per wave (a workgroup owns 64 RT rows): every fragment of up feeds RT MFMAs
template <int T_ID, int RT>
__global__ __launch_bounds__(256) void lowrank_add_kernel(const uint16_t* __restrict__ t, const uint16_t* __restrict__ up,
                                                          uint16_t* __restrict__ y, int64_t M, int64_t N, int64_t ldy, int R, float scale) {
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
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // a sum that is exactly zero leaves the element as it is: fmaf(scale, +0, -0.0) is +0.0
                    const float a0 = acc[r][c][0][e], a1 = acc[r][c][1][e];
                    f[e] = a0 == 0.0f ? f[e] : fmaf(scale, a0, f[e]);
                    f[4 + e] = a1 == 0.0f ? f[4 + e] : fmaf(scale, a1, f[4 + e]);
                }
                *p = Vec16<T_ID>::pack(f);
            }
        }
    }
}

// ---- out = scale * a^T . b ------------------------------------------------------------------------------------------------------------
// NRT: rank tiles of 16 (rank <= 16 NRT).  grid (column tiles of a, slabs).  `direct`: one slab -- scale, round and store out; otherwise
// the float32 partial goes to part [slab][P][R].
template <bool IS_BF16, int NRT>
__global__ __launch_bounds__(256) void lowrank_grad_kernel(const uint16_t* __restrict__ a, int64_t lda, const uint16_t* __restrict__ b,
                                                           int64_t M, int64_t P, int R, float scale, int out_t, void* __restrict__ out,
                                                           int out_dtype, float* __restrict__ part, int direct) {
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

}  // namespace

extern "C" int sdnq_hip_lowrank_add(const void* t, const void* up, int dtype, int rank, float scale, void* y, int64_t m, int64_t n,
                                    int64_t ldy, sdnq_stream_t stream) {
    if (!t || !up || !y) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (m <= 0 || n <= 0 || ldy < n || (n % 8) != 0 || rank < 8 || rank > 256 || (rank % 8) != 0) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)t % 16) || ((uintptr_t)up % 16) || ((uintptr_t)y % 16) || ((ldy * 2) % 16)) return SDNQ_ERR_ALIGN;
    // two row tiles per wave halve the fragment loads of up per element of y; taken once the launch still has two workgroups per CU
    const int64_t gx = (n + 127) / 128;
    const bool two = gx * ((m + 127) / 128) >= 512;
    const int64_t gy = two ? (m + 127) / 128 : (m + 63) / 64;
    if (gx > 0x7fffffff || gy > 65535) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)t, (const uint16_t*)up, (uint16_t*)y, m, n, ldy, rank, scale);
    };
    if (dtype == SDNQ_BF16) { if (two) launch(lowrank_add_kernel<SDNQ_BF16, 2>); else launch(lowrank_add_kernel<SDNQ_BF16, 1>); }
    else { if (two) launch(lowrank_add_kernel<SDNQ_F16, 2>); else launch(lowrank_add_kernel<SDNQ_F16, 1>); }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int64_t sdnq_hip_lowrank_grad_workspace_bytes(int64_t m, int64_t p, int rank) {
    if (m <= 0 || p <= 0 || (p % 8) != 0 || rank < 8 || rank > 256 || (rank % 8) != 0) return SDNQ_ERR_SHAPE;
    const int64_t slabs = (m + LRG_SLAB - 1) / LRG_SLAB;
    return slabs <= 1 ? 0 : slabs * p * rank * 4;
}

extern "C" int sdnq_hip_lowrank_grad(const void* a, int64_t lda, const void* b, int dtype, int64_t m, int64_t p, int rank, float scale,
                                     int out_t, void* out, int out_dtype, void* workspace, int64_t workspace_bytes, sdnq_stream_t stream) {
    if (!a || !b || !out) return SDNQ_ERR_NULL;
    if ((dtype != SDNQ_BF16 && dtype != SDNQ_F16) || out_dtype < 0 || out_dtype > 2) return SDNQ_ERR_DTYPE;
    if (m <= 0 || p <= 0 || lda < p || (p % 8) != 0 || rank < 8 || rank > 256 || (rank % 8) != 0 || (out_t != 0 && out_t != 1)) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)a % 16) || ((uintptr_t)b % 16) || ((lda * 2) % 16) || ((uintptr_t)out % (out_dtype == SDNQ_F32 ? 4 : 2))) return SDNQ_ERR_ALIGN;
    const int64_t need = sdnq_hip_lowrank_grad_workspace_bytes(m, p, rank);
    const int64_t slabs = (m + LRG_SLAB - 1) / LRG_SLAB;
    if (need > 0) {
        if (!workspace) return SDNQ_ERR_NULL;
        if (workspace_bytes < need) return SDNQ_ERR_SHAPE;
        if ((uintptr_t)workspace % 16) return SDNQ_ERR_ALIGN;
    }
    const int64_t gx = (p + 63) / 64, total = p * rank;
    if (gx > 0x7fffffff || slabs > 65535 || (total + 255) / 256 > 0x7fffffff) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)slabs), block(256);
    hipStream_t s = (hipStream_t)stream;
    const int direct = slabs == 1;
    float* part = (float*)workspace;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)a, lda, (const uint16_t*)b, m, p, rank, scale, out_t, out, out_dtype, part, direct);
    };
    const bool bf = dtype == SDNQ_BF16;
    if (rank <= 16) { if (bf) launch(lowrank_grad_kernel<true, 1>); else launch(lowrank_grad_kernel<false, 1>); }
    else if (rank <= 32) { if (bf) launch(lowrank_grad_kernel<true, 2>); else launch(lowrank_grad_kernel<false, 2>); }
    else if (rank <= 64) { if (bf) launch(lowrank_grad_kernel<true, 4>); else launch(lowrank_grad_kernel<false, 4>); }
    else if (rank <= 128) { if (bf) launch(lowrank_grad_kernel<true, 8>); else launch(lowrank_grad_kernel<false, 8>); }
    else { if (bf) launch(lowrank_grad_kernel<true, 16>); else launch(lowrank_grad_kernel<false, 16>); }
    SDNQ_CHECK_LAUNCH();
    if (!direct) {
        hipLaunchKernelGGL(lowrank_grad_sum_kernel, dim3((unsigned)((total + 255) / 256)), block, 0, s, (const float*)part, slabs, p, rank, scale,
                           out_t, out, out_dtype);
        SDNQ_CHECK_LAUNCH();
    }
    return SDNQ_OK;
}
