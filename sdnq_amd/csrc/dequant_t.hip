// The weight operand of grad_input = dY . W for a frozen quantized Linear layer (QuantizedLinearBackward, training/layers/linear/forward.py:
// grad_output @ weight.dequantize()): the product reduces over N, and the float GEMM (linear_float.hip) wants both operands contiguous
// along the reduction, so the weight is needed as [K][N].
//
//   sdnq_hip_dequant_t   the stored codes decoded straight into that operand: out[k][n] = the value sdnq_hip_dequant writes to out[n][k],
//       bit for bit, for a weight without SVD factors and with no Hadamard rotation.  The per-element arithmetic IS dequant16 (weight_dev.h):
//       every storage format, group scales, zero points, codebooks, the one rounding to a 16-bit scale dtype.  A workgroup takes 64 rows
//       (n) x 64 columns (k) of the stored matrix: thread t decodes the 16-run (row t / 4, run t % 4), the tile crosses LDS and leaves as
//       16-byte runs along n (4 float32 or 8 16-bit values per lane, a 64-value row of the tile = 256 / 128 contiguous bytes of out).
//       LDS image: float tile[64 k][64 n], the n index XOR-ed with swz(k) = 8 * (k / 16) + 4 * ((k / 2) % 2).
//         stores (ds_write_b32, banks = dword % 32, conflicts inside a 32-lane half): in one store instruction j is the same for every
//           lane, the half holds 8 consecutive rows (n = 8a .. 8a + 7) x the 4 runs; the runs differ in k / 16, so their XOR terms 0, 8, 16,
//           24 send them to four disjoint 8-bank ranges: conflict-free (the unswizzled [64][64] image would be 4-way, a [64][65] one 2-way).
//         loads (ds_read_b128, banks = dword % 64, conflicts inside the four 16-lane groups of MI355X_MICROARCH.md, LDS): a row of the image is
//           exactly the 64 banks.  float32 output: a group reads the 16 quads of two rows k = 2a, 2a + 1, eight from each, complementary
//           quad ranges; both rows have the same swz, a permutation of the quads: conflict-free.  16-bit output: a lane reads quads
//           2p, 2p + 1 of its row in two loads; a group holds quads {0, 2, 4, 6} of rows 4a and 4a + 3 and {8, 10, 12, 14} of rows 4a + 1
//           and 4a + 2 (or the complement); the 4 * ((k / 2) % 2) term moves rows 4a + 2, 4a + 3 to the odd quads: conflict-free.
//       The bank arithmetic above is worked out by hand from the guide's tables; no counter run has confirmed it.
//       Scale / zero point are read as dequant16 reads them (per 16-run, from L1 / L2 after a tile's first row): untuned.
//
//   sdnq_hip_transpose2d  a plain tiled transpose of a float matrix, [r][c] (row stride ldx) -> [c][r]: the route of layers with SVD factors
//       or a Hadamard rotation, whose full weight sdnq_hip_dequant writes first.  64 x 64 tile, 16-byte loads along c, element stores into a
//       padded LDS image, 16-byte runs along r out.  One extra pass over the weight; untuned (2-byte LDS stores for 16-bit elements).
#include "weight_dev.h"

namespace {

__device__ __forceinline__ int tile_swz(int k) { return ((k >> 4) << 3) | (((k >> 1) & 1) << 2); }

template <int T_ID>
__global__ __launch_bounds__(256) void dequant_t_kernel(const DeqParams p, void* __restrict__ out) {
    constexpr int VN = Vec16<T_ID>::n, CH = 64 / VN;
    __shared__ __attribute__((aligned(16))) float tile[64][64];  // [k][n ^ swz(k)]
    const int tid = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * 64, n0 = (int64_t)blockIdx.y * 64;
    {
        const int r = tid >> 2, ch = tid & 3;
        const int64_t n = n0 + r, k = k0 + ch * 16;
        if (n < p.N && k < p.K) {  // K % 16 == 0: a run of 16 never leaves its row
            float v[16];
            dequant16(p, n, k, v);
#pragma unroll
            for (int j = 0; j < 16; ++j) tile[ch * 16 + j][r ^ tile_swz(ch * 16 + j)] = v[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int o = tid; o < 64 * CH; o += 256) {
        const int kl = o / CH, cc = (o % CH) * VN;
        const int64_t k = k0 + kl, n = n0 + cc;
        if (k < p.K && n < p.N) {  // N % 8 == 0: a run of VN values stays inside the row of out, 16-byte aligned
            float f[VN];
#pragma unroll
            for (int q = 0; q < VN; q += 4) {
                const float4 t = *(const float4*)&tile[kl][(cc + q) ^ tile_swz(kl)];
                f[q] = t.x; f[q + 1] = t.y; f[q + 2] = t.z; f[q + 3] = t.w;
            }
            *(uint4*)((uint8_t*)out + (k * p.N + n) * FT<T_ID>::bytes) = Vec16<T_ID>::pack(f);
        }
    }
}

// E: the element as an unsigned integer of its size (the values are moved, never read as numbers)
template <typename E>
__global__ __launch_bounds__(256) void transpose2d_kernel(const E* __restrict__ x, int64_t R, int64_t C, int64_t ldx, E* __restrict__ out) {
    constexpr int VN = 16 / (int)sizeof(E), CH = 64 / VN;
    __shared__ __attribute__((aligned(16))) E tile[64][64 + VN];  // [c][r]; rows of 16-byte multiples
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
#pragma unroll
    for (int o = tid; o < 64 * CH; o += 256) {
        const int rl = o / CH, cc = (o % CH) * VN;
        const int64_t r = r0 + rl, c = c0 + cc;
        if (r < R && c < C) {  // C % 8 == 0: a run of VN elements stays inside the row
            const uint4 v = *(const uint4*)(x + r * ldx + c);
            E e[VN];
            __builtin_memcpy(e, &v, 16);
#pragma unroll
            for (int i = 0; i < VN; ++i) tile[cc + i][rl] = e[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int o = tid; o < 64 * CH; o += 256) {
        const int cl = o / CH, rr = (o % CH) * VN;
        const int64_t c = c0 + cl, r = r0 + rr;
        if (c < C && r < R) *(uint4*)(out + c * R + r) = *(const uint4*)&tile[cl][rr];  // R % 8 == 0
    }
}

}  // namespace

extern "C" int sdnq_hip_dequant_t(const SdnqWeight* w, void* out, int out_dtype, sdnq_stream_t stream) {
    DeqParams p{};
    const int st = fill_params(w, p);  // NULL, formats, group shape, code alignment
    // (fill_params calls K % 16 != 0 a shape error: no entry point reads such a weight; here it is a Linear layer this kernel is not built for)
    if (st == SDNQ_ERR_SHAPE && w->k > 0 && (w->k % 16) != 0) return SDNQ_ERR_UNSUPPORTED;
    if (st != SDNQ_OK) return st;
    if (!out) return SDNQ_ERR_NULL;
    if (out_dtype < 0 || out_dtype > 2) return SDNQ_ERR_DTYPE;
    if (p.svd_up || (p.N % 8) != 0) return SDNQ_ERR_UNSUPPORTED;
    if ((uintptr_t)out % 16) return SDNQ_ERR_ALIGN;
    const int64_t gx = (p.K + 63) / 64, gy = (p.N + 63) / 64;
    if (gy > 65535) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    hipStream_t s = (hipStream_t)stream;
    dispatch_float(out_dtype, [&](auto O) {
        hipLaunchKernelGGL((dequant_t_kernel<O.value>), grid, block, 0, s, p, out);
        return true;
    });
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_transpose2d(const void* x, int dtype, int64_t r, int64_t c, int64_t ldx, void* out, sdnq_stream_t stream) {
    if (!x || !out) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    if (r <= 0 || c <= 0 || ldx < c || (r % 8) != 0 || (c % 8) != 0) return SDNQ_ERR_SHAPE;
    const int eb = dtype == SDNQ_F32 ? 4 : 2;
    if ((uintptr_t)x % 16 || (uintptr_t)out % 16 || (ldx * eb) % 16) return SDNQ_ERR_ALIGN;
    const int64_t gx = (c + 63) / 64, gy = (r + 63) / 64;
    if (gx > 0x7fffffff || gy > 65535) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (eb == 4) hipLaunchKernelGGL((transpose2d_kernel<uint32_t>), grid, block, 0, s, (const uint32_t*)x, r, c, ldx, (uint32_t*)out);
    else hipLaunchKernelGGL((transpose2d_kernel<uint16_t>), grid, block, 0, s, (const uint16_t*)x, r, c, ldx, (uint16_t*)out);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
