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
#include "philox_dev.h"   // dropout_chunk, dropout_keep8: the masks of the _dropout entry points

namespace {

constexpr int LRG_SLAB = 256;  // rows of M per partial sum of sdnq_hip_lowrank_grad (tests/lora_util.py restates it)

// The kernels' text lives in lowrank_add_kernel.h and lowrank_grad_kernel.h, each included once per form: the plain kernel (LR_DROP 0) and
// the _dropout one (LR_DROP 1: sdnq_hip_lowrank_add_dropout, sdnq_hip_lowrank_grad_dropout); the add kernel a third time for DoRA's
// epilogue (LR_DORA 1: sdnq_hip_lowrank_add_dora).
// ---- y += scale * t . up^T ------------------------------------------------------------------------------------------------------------
#define LR_DORA 0
#define LR_DROP 0
#include "lowrank_add_kernel.h"
#undef LR_DROP
#define LR_DROP 1
#include "lowrank_add_kernel.h"
#undef LR_DROP
#undef LR_DORA
#define LR_DORA 1
#define LR_DROP 0
#include "lowrank_add_kernel.h"
#undef LR_DROP
#undef LR_DORA

// ---- out = scale * a^T . b ------------------------------------------------------------------------------------------------------------
#define LR_DROP 0
#include "lowrank_grad_kernel.h"
#undef LR_DROP
#define LR_DROP 1
#include "lowrank_grad_kernel.h"
#undef LR_DROP

}  // namespace

// drop == nullptr: the plain kernels; c != nullptr: the DoRA epilogue (no mask: its dropout lives in t)
static int lowrank_add_launch(const void* t, const void* up, int dtype, int rank, float scale, void* y, int64_t m, int64_t n, int64_t ldy,
                              const DropArgs* drop, sdnq_stream_t stream, const float* c = nullptr, const void* bias = nullptr) {
    if (!t || !up || !y) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    if (m <= 0 || n <= 0 || ldy < n || (n % 8) != 0 || rank < 8 || rank > 256 || (rank % 8) != 0) return SDNQ_ERR_SHAPE;
    if (drop && (drop->thr < 1u || drop->thr > 65535u)) return SDNQ_ERR_SHAPE;  // (a negative threshold arrives as a large unsigned one)
    if (((uintptr_t)t % 16) || ((uintptr_t)up % 16) || ((uintptr_t)y % 16) || ((ldy * 2) % 16)) return SDNQ_ERR_ALIGN;
    if (((uintptr_t)c % 16) || ((uintptr_t)bias % 16)) return SDNQ_ERR_ALIGN;
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
    auto launch_drop = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)t, (const uint16_t*)up, (uint16_t*)y, m, n, ldy, rank, scale, drop->thr,
                           drop->seed_lo, drop->seed_hi, drop->off_lo, drop->off_hi);
    };
    auto launch_dora = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)t, (const uint16_t*)up, (uint16_t*)y, m, n, ldy, rank, scale, c,
                           (const uint16_t*)bias);
    };
    if (c) {
        if (dtype == SDNQ_BF16) { if (two) launch_dora(lowrank_add_dora_kernel<SDNQ_BF16, 2>); else launch_dora(lowrank_add_dora_kernel<SDNQ_BF16, 1>); }
        else { if (two) launch_dora(lowrank_add_dora_kernel<SDNQ_F16, 2>); else launch_dora(lowrank_add_dora_kernel<SDNQ_F16, 1>); }
    } else if (drop) {
        if (dtype == SDNQ_BF16) { if (two) launch_drop(lowrank_add_dropout_kernel<SDNQ_BF16, 2>); else launch_drop(lowrank_add_dropout_kernel<SDNQ_BF16, 1>); }
        else { if (two) launch_drop(lowrank_add_dropout_kernel<SDNQ_F16, 2>); else launch_drop(lowrank_add_dropout_kernel<SDNQ_F16, 1>); }
    } else if (dtype == SDNQ_BF16) { if (two) launch(lowrank_add_kernel<SDNQ_BF16, 2>); else launch(lowrank_add_kernel<SDNQ_BF16, 1>); }
    else { if (two) launch(lowrank_add_kernel<SDNQ_F16, 2>); else launch(lowrank_add_kernel<SDNQ_F16, 1>); }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_lowrank_add(const void* t, const void* up, int dtype, int rank, float scale, void* y, int64_t m, int64_t n,
                                    int64_t ldy, sdnq_stream_t stream) {
    return lowrank_add_launch(t, up, dtype, rank, scale, y, m, n, ldy, nullptr, stream);
}

extern "C" int sdnq_hip_lowrank_add_dropout(const void* t, const void* up, int dtype, int rank, float scale, void* y, int64_t m, int64_t n,
                                            int64_t ldy, int threshold, uint64_t seed, uint64_t offset, sdnq_stream_t stream) {
    const DropArgs drop = {(u32)threshold, (u32)seed, (u32)(seed >> 32), (u32)offset, (u32)(offset >> 32)};
    return lowrank_add_launch(t, up, dtype, rank, scale, y, m, n, ldy, &drop, stream);
}

extern "C" int sdnq_hip_lowrank_add_dora(const void* t, const void* up, int dtype, int rank, float scale, void* y, int64_t m, int64_t n,
                                         int64_t ldy, const float* c, const void* bias, sdnq_stream_t stream) {
    if (!c) return SDNQ_ERR_NULL;
    return lowrank_add_launch(t, up, dtype, rank, scale, y, m, n, ldy, nullptr, stream, c, bias);
}

extern "C" int64_t sdnq_hip_lowrank_grad_workspace_bytes(int64_t m, int64_t p, int rank) {
    if (m <= 0 || p <= 0 || (p % 8) != 0 || rank < 8 || rank > 256 || (rank % 8) != 0) return SDNQ_ERR_SHAPE;
    const int64_t slabs = (m + LRG_SLAB - 1) / LRG_SLAB;
    return slabs <= 1 ? 0 : slabs * p * rank * 4;
}

// drop == nullptr: the plain kernels
static int lowrank_grad_launch(const void* a, int64_t lda, const void* b, int dtype, int64_t m, int64_t p, int rank, float scale, int out_t,
                               void* out, int out_dtype, void* workspace, int64_t workspace_bytes, const DropArgs* drop, sdnq_stream_t stream) {
    if (!a || !b || !out) return SDNQ_ERR_NULL;
    if ((dtype != SDNQ_BF16 && dtype != SDNQ_F16) || out_dtype < 0 || out_dtype > 2) return SDNQ_ERR_DTYPE;
    if (m <= 0 || p <= 0 || lda < p || (p % 8) != 0 || rank < 8 || rank > 256 || (rank % 8) != 0 || (out_t != 0 && out_t != 1)) return SDNQ_ERR_SHAPE;
    if (drop && (drop->thr < 1u || drop->thr > 65535u)) return SDNQ_ERR_SHAPE;  // (a negative threshold arrives as a large unsigned one)
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
    auto launch_drop = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)a, lda, (const uint16_t*)b, m, p, rank, scale, out_t, out, out_dtype, part, direct,
                           drop->thr, drop->seed_lo, drop->seed_hi, drop->off_lo, drop->off_hi);
    };
    const bool bf = dtype == SDNQ_BF16;
    if (drop) {
        if (rank <= 16) { if (bf) launch_drop(lowrank_grad_dropout_kernel<true, 1>); else launch_drop(lowrank_grad_dropout_kernel<false, 1>); }
        else if (rank <= 32) { if (bf) launch_drop(lowrank_grad_dropout_kernel<true, 2>); else launch_drop(lowrank_grad_dropout_kernel<false, 2>); }
        else if (rank <= 64) { if (bf) launch_drop(lowrank_grad_dropout_kernel<true, 4>); else launch_drop(lowrank_grad_dropout_kernel<false, 4>); }
        else if (rank <= 128) { if (bf) launch_drop(lowrank_grad_dropout_kernel<true, 8>); else launch_drop(lowrank_grad_dropout_kernel<false, 8>); }
        else { if (bf) launch_drop(lowrank_grad_dropout_kernel<true, 16>); else launch_drop(lowrank_grad_dropout_kernel<false, 16>); }
    } else if (rank <= 16) { if (bf) launch(lowrank_grad_kernel<true, 1>); else launch(lowrank_grad_kernel<false, 1>); }
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

extern "C" int sdnq_hip_lowrank_grad(const void* a, int64_t lda, const void* b, int dtype, int64_t m, int64_t p, int rank, float scale,
                                     int out_t, void* out, int out_dtype, void* workspace, int64_t workspace_bytes, sdnq_stream_t stream) {
    return lowrank_grad_launch(a, lda, b, dtype, m, p, rank, scale, out_t, out, out_dtype, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int sdnq_hip_lowrank_grad_dropout(const void* a, int64_t lda, const void* b, int dtype, int64_t m, int64_t p, int rank, float scale,
                                             int out_t, void* out, int out_dtype, void* workspace, int64_t workspace_bytes, int threshold,
                                             uint64_t seed, uint64_t offset, sdnq_stream_t stream) {
    const DropArgs drop = {(u32)threshold, (u32)seed, (u32)(seed >> 32), (u32)offset, (u32)(offset >> 32)};
    return lowrank_grad_launch(a, lda, b, dtype, m, p, rank, scale, out_t, out, out_dtype, workspace, workspace_bytes, &drop, stream);
}
