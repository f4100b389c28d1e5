// Column-wise int8 quantization with TRANSPOSED codes for gfx950: the operand preparation of the training Linear's two backward matmuls.
//
// Reference chain replaced (five elementwise / reduction passes plus a transposing copy there; TWO launches here):
//   scale = amax(|x|, dim=0) / 127                         quant_utils.py:23-24, 268
//   q = clamp(round(x / scale), -128, 127).to(int8)        quant_utils.py:269-272   (quantize_int_mm(.., dim=0))
//   as called on the weight   W [N][K]  of grad_input      linear_int8_dynamic.py:27, linear_int8_dynamic_ckpt.py:22
//   and on the input          x [M][K]  of grad_weight     linear_int8_dynamic.py:27 (weight = input.flatten(0,-2)), _ckpt.py:26
//   and, as quantize_int_mm(dY.t(), dim=-1), on dY [M][N]  linear_int8_dynamic.py:28
//   grad_bias = grad_output.sum(dim=0)                     linear_int8_dynamic.py:153          (colsum, optional)
// The matmul that follows (sdnq_hip_scaled_mm) reduces over the ROW index of x, so the codes leave as xq_t [C][ld_t]: column c of x is
// row c of the operand, zero-padded to ld_t (a multiple of 16, the GEMM's K granularity).
//
// Two kernels, no atomics (bit-identical from run to run):
//   colstat_kernel     a block = 64 columns x one slab of rows.  Lane = 8 consecutive columns (one 16-byte load for 16-bit inputs), 32
//                      rows per pass; per-column |max| and sum stay in registers down the slab, the 32 row groups of the block meet in
//                      LDS in a fixed order, one partial per (slab, column) goes to the workspace.
//   colquant_t_kernel  a block = 64 columns x 256 rows.  Reduces the <= 32 slab partials of its columns (fixed order), then quantizes its
//                      tile: each lane holds 4 consecutive ROWS of 8 columns, so the four codes of a column are one dword and the LDS
//                      transpose is written with ds_write_b32 (16-byte chunks XOR-swizzled by column group: a wave's 64 lanes cover 32
//                      distinct banks; bank conflicts have not been measured), read back as 16-byte chunks along the row index and
//                      stored 16 bytes per lane, 256 contiguous bytes per 16 lanes.
// Traffic for a 16-bit input: 2 reads of x + 1 write of codes = 5 B per element, plus 8 B x C x slabs of partials: written once (at most
// 256 B per column), re-read by every row tile for its 64 columns (up to 16 KiB per tile; expected in L2, not measured).
// NaN: fmaxf drops a NaN operand, so a NaN in x does not reach the scale (torch's amax would propagate it).  This is
// sdnq_hip_rowquant's convention; the reference's result for such a column is a NaN cast to int8, which is undefined.  An inf makes its
// column's scale inf: every finite element gets code 0 and the inf itself (inf / inf) -128, again as sdnq_hip_rowquant has it
// (tests/test_colquant_exact_gpu.py holds the two kernels to each other on NaN, +inf, -inf and all-zero columns).
#include "quant8_dev.h"
#include "sdnq_dev.h"

namespace {

constexpr int CQ_CT = 64;    // columns per block
constexpr int CQ_RT = 256;   // rows per block of the quantize kernel
constexpr int CQ_MAX_SLABS = 32;

// 8 consecutive elements of row-major x at element index `idx` (a lane that is masked out re-reads the start of x, see load8_raw in rowquant.hip)
template <int T_ID>
__device__ __forceinline__ void cq_load8(const void* x, int64_t idx, uint4& a, uint4& b) {
    if constexpr (T_ID == SDNQ_F32) {
        a = *(const uint4*)((const float*)x + idx);
        b = *(const uint4*)((const float*)x + idx + 4);
    } else {
        a = *(const uint4*)((const uint16_t*)x + idx);
        b = a;
    }
}
template <int T_ID>
__device__ __forceinline__ void cq_unpack8(const uint4& a, const uint4& b, bool ok, float (&v)[8]) {
    if constexpr (T_ID == SDNQ_F32) {
        Vec16<SDNQ_F32>::unpack(a, v);
        Vec16<SDNQ_F32>::unpack(b, v + 4);
    } else {
        Vec16<T_ID>::unpack(a, v);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ok ? v[e] : 0.0f;
}

// grid (column tiles, slabs); part_amax / part_sum: [slabs][C]
template <int T_ID>
__global__ __launch_bounds__(256) void colstat_kernel(const void* __restrict__ x, int64_t R, int64_t C, int64_t ldx, int64_t slab_rows,
                                                      float* __restrict__ part_amax, float* __restrict__ part_sum) {
    __shared__ float s_amax[32][CQ_CT];
    __shared__ float s_sum[32][CQ_CT];
    const int cg = threadIdx.x & 7, rr = threadIdx.x >> 3;
    const int64_t c0 = (int64_t)blockIdx.x * CQ_CT + cg * 8;
    const bool col_ok = c0 < C;
    const int64_t r_begin = (int64_t)blockIdx.y * slab_rows;
    const int64_t r_end = (r_begin + slab_rows < R) ? r_begin + slab_rows : R;
    float amax[8], sum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { amax[e] = 0.0f; sum[e] = 0.0f; }
    for (int64_t r = r_begin + rr; r < r_begin + slab_rows; r += 32 * 4) {  // four passes' loads in flight
        uint4 ra[4], rb[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ok[u] = col_ok && r + 32 * u < r_end;
            cq_load8<T_ID>(x, ok[u] ? (r + 32 * u) * ldx + c0 : 0, ra[u], rb[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v[8];
            cq_unpack8<T_ID>(ra[u], rb[u], ok[u], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { amax[e] = fmaxf(amax[e], fabsf(v[e])); sum[e] += v[e]; }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { s_amax[rr][cg * 8 + e] = amax[e]; s_sum[rr][cg * 8 + e] = sum[e]; }
    __syncthreads();
    if (threadIdx.x < CQ_CT) {
        const int64_t c = (int64_t)blockIdx.x * CQ_CT + threadIdx.x;
        float a = 0.0f, s = 0.0f;
#pragma unroll 8
        for (int q = 0; q < 32; ++q) { a = fmaxf(a, s_amax[q][threadIdx.x]); s += s_sum[q][threadIdx.x]; }
        if (c < C) {
            part_amax[(int64_t)blockIdx.y * C + c] = a;
            part_sum[(int64_t)blockIdx.y * C + c] = s;
        }
    }
}

// grid (column tiles, ceil(ld_t / 256)); rows [R, ld_t) of the operand are written as zeros
template <int T_ID>
__global__ __launch_bounds__(256) void colquant_t_kernel(const void* __restrict__ x, int64_t R, int64_t C, int64_t ldx, int nslab,
                                                         const float* __restrict__ part_amax, const float* __restrict__ part_sum,
                                                         uint8_t* __restrict__ xq_t, int64_t ld_t, float* __restrict__ xs,
                                                         float* __restrict__ colsum) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[CQ_CT * CQ_RT];  // [column][row], 16-byte chunks XOR-swizzled by column group
    __shared__ float s_scale[CQ_CT];
    __shared__ float s_rcp[CQ_CT];
    __shared__ int s_fast[CQ_CT];
    const int tid = threadIdx.x;
    const int cg = tid & 7, rg = tid >> 3;  // 8 columns, 4 rows per lane and step; two steps of 128 rows
    const int64_t c0 = (int64_t)blockIdx.x * CQ_CT + cg * 8;
    const bool col_ok = c0 < C;
    const int64_t r0 = (int64_t)blockIdx.y * CQ_RT;
    // the tile's loads go out first: the partial reduction below runs under their latency
    uint4 ra[2][4], rb[2][4];
    bool ok[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + s * 128 + rg * 4 + j;
            ok[s][j] = col_ok && r < R;
            cq_load8<T_ID>(x, ok[s][j] ? r * ldx + c0 : 0, ra[s][j], rb[s][j]);
        }
    }
    if (tid < CQ_CT) {  // scale of column c: slab partials in slab order
        const int64_t c = (int64_t)blockIdx.x * CQ_CT + tid;
        float a = 0.0f;
        if (c < C) {
            for (int q = 0; q < nslab; ++q) a = fmaxf(a, part_amax[(int64_t)q * C + c]);
        }
        const float scale = a / 127.0f;  // IEEE division (get_scale_symmetric, quant_utils.py:23-24)
        RowDiv rd;
        rd.set(scale);
        s_scale[tid] = scale;
        s_rcp[tid] = rd.rcp;
        s_fast[tid] = rd.fast ? 1 : 0;
        if (blockIdx.y == 0 && c < C) xs[c] = scale;
    } else if (tid < 2 * CQ_CT && blockIdx.y == 0 && colsum != nullptr) {
        const int64_t c = (int64_t)blockIdx.x * CQ_CT + (tid - CQ_CT);
        if (c < C) {
            float s = 0.0f;
            for (int q = 0; q < nslab; ++q) s += part_sum[(int64_t)q * C + c];
            colsum[c] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float v[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j) cq_unpack8<T_ID>(ra[s][j], rb[s][j], ok[s][j], v[j]);
        const int row = s * 128 + rg * 4;  // first of this lane's 4 rows inside the tile
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int cl = cg * 8 + e;
            RowDiv rd;
            rd.scale = s_scale[cl];
            rd.rcp = s_rcp[cl];
            u32 w;
            // per column, so per lane: a wave whose 8 column groups mix ordinary columns with all-zero or out-of-range ones runs both
            // branches (quant8 in rowquant.hip has one row per wave and never does); the bits are the same either way
            if (s_fast[cl]) {  // the arithmetic of the row quantizer (quant8_fast): correctly rounded quotient, rint and int8 cast as one packed add
                w = pack4_rne_i8(fastdiv2((pv2f){v[0][e], v[1][e]}, rd), fastdiv2((pv2f){v[2][e], v[3][e]}, rd));
            } else {  // scale 0 (an all-zero column: codes 0, as sdnq_hip_rowquant defines it), inf / nan, or outside the fast range
                w = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // the row quantizer's expression as it stands (quant8 in quant8_dev.h), so a NaN quotient -- +-inf under the scale inf
                    // of its own column -- leaves the clamp as -128 here as it does there, not as a code of this kernel's own
                    float q = (rd.scale == 0.0f) ? 0.0f : __builtin_rintf(v[j][e] / rd.scale);
                    q = fminf(fmaxf(q, -128.0f), 127.0f);
                    w |= ((u32)(int)q & 0xffu) << (8 * j);
                }
            }
            *(u32*)(s_tile + cl * CQ_RT + ((((row >> 4) ^ cg) << 4) | (row & 15))) = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k;
        const int cl = i >> 4, chunk = i & 15;
        const int64_t c = (int64_t)blockIdx.x * CQ_CT + cl;
        const int64_t r = r0 + chunk * 16;
        if (c < C && r < ld_t) *(uint4*)(xq_t + c * ld_t + r) = *(const uint4*)(s_tile + cl * CQ_RT + ((chunk ^ (cl >> 3)) << 4));
    }
}

// how the rows are cut into slabs for the statistics pass: enough blocks to fill the chip at few rows, at most 32 partials per column
void cq_plan(int64_t r, int64_t c, int64_t& ctiles, int64_t& nslab, int64_t& slab_rows) {
    ctiles = (c + CQ_CT - 1) / CQ_CT;
    int64_t want = (512 + ctiles - 1) / ctiles;
    if (want > CQ_MAX_SLABS) want = CQ_MAX_SLABS;
    const int64_t by_rows = (r + 31) / 32;
    nslab = want < by_rows ? want : by_rows;
    slab_rows = ((r + nslab - 1) / nslab + 127) / 128 * 128;  // a multiple of the 128 rows one block iteration covers
    nslab = (r + slab_rows - 1) / slab_rows;
}

}  // namespace

extern "C" int64_t sdnq_hip_colquant_t_workspace_bytes(int64_t r, int64_t c) {
    if (r <= 0 || c <= 0 || (c % 8) != 0) return SDNQ_ERR_SHAPE;
    int64_t ctiles, nslab, slab_rows;
    cq_plan(r, c, ctiles, nslab, slab_rows);
    return 2 * nslab * c * (int64_t)sizeof(float);
}

extern "C" int sdnq_hip_colquant_t(const void* x, int x_dtype, int64_t r, int64_t c, int64_t ldx, void* xq_t, int64_t ld_t, float* xs,
                                   float* colsum, void* workspace, int64_t workspace_bytes, sdnq_stream_t stream) {
    if (!x || !xq_t || !xs || !workspace) return SDNQ_ERR_NULL;
    if (x_dtype < 0 || x_dtype > 2) return SDNQ_ERR_DTYPE;
    if (r <= 0 || c <= 0 || (c % 8) != 0 || ldx < c || ld_t < r || (ld_t % 16) != 0) return SDNQ_ERR_SHAPE;
    const int eb = (x_dtype == SDNQ_F32) ? 4 : 2;
    if (((uintptr_t)x % 16) || ((ldx * eb) % 16) || ((uintptr_t)xq_t % 16) || ((uintptr_t)workspace % 16)) return SDNQ_ERR_ALIGN;
    int64_t ctiles, nslab, slab_rows;
    cq_plan(r, c, ctiles, nslab, slab_rows);
    if (workspace_bytes < 2 * nslab * c * (int64_t)sizeof(float)) return SDNQ_ERR_SHAPE;
    const int64_t rtiles = (ld_t + CQ_RT - 1) / CQ_RT;
    if (ctiles > 0x7fffffff || rtiles > 65535) return SDNQ_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    float* part_amax = (float*)workspace;
    float* part_sum = part_amax + nslab * c;
    const dim3 block(256), grid1((unsigned)ctiles, (unsigned)nslab), grid2((unsigned)ctiles, (unsigned)rtiles);
#define CQ_LAUNCH(T)                                                                                                              \
    do {                                                                                                                          \
        hipLaunchKernelGGL((colstat_kernel<T>), grid1, block, 0, s, x, r, c, ldx, slab_rows, part_amax, part_sum);                \
        hipLaunchKernelGGL((colquant_t_kernel<T>), grid2, block, 0, s, x, r, c, ldx, (int)nslab, (const float*)part_amax,         \
                           (const float*)part_sum, (uint8_t*)xq_t, ld_t, xs, colsum);                                             \
    } while (0)
    switch (x_dtype) {
        case SDNQ_F32: CQ_LAUNCH(SDNQ_F32); break;
        case SDNQ_BF16: CQ_LAUNCH(SDNQ_BF16); break;
        default: CQ_LAUNCH(SDNQ_F16); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
