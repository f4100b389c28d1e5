// Trainable low-rank adapters (LoRA) on frozen quantized Conv1d / Conv2d layers: the two products of the adapter branch that read the
// UNFOLDED activation im2col(x) [B OH OW][C kh kw] -- as implicit GEMMs on x [B][C][H][W] itself, so that the unfolded matrix (kh kw
// times the bytes of x) is never written.  No reference interface: the reference has no adapters.
//
//   sdnq_hip_conv_lowrank_down   t = im2col(x) . down^T, the adapter's down projection (PEFT's lora_A, a conv with the layer's geometry):
//       t[(b, oh, ow)][r] = round_dtype( sum_{c,i,j} x[b][c][oh s_h - p_h + i d_h][ow s_w - p_w + j d_w] * down[r][(c kh + i) kw + j] )
//       A workgroup owns 16 consecutive output positions and every rank column; K = C kh kw is cut into chunks of 64 columns that go round
//       its waves (16 of them up to rank 64; 4 beyond, where the accumulators take the registers -- those ranks are not measured).  Per chunk a wave writes the 64 x 16 window of im2col(x) to an LDS
//       image [k][position] of its own -- the fast axis is the output position, along which x is contiguous (stride 1); the taps a position
//       shares with its neighbours and with the other chunks are re-read from L1 / L2, not from HBM -- and takes the MFMA operand (8
//       consecutive k per lane) out of it transposed by ds_read_b64_tr_b16 (lrg_frag of lowrank_dev.h, the 32-byte rows of
//       lowrank_grad's narrowest image).  The other operand, 16 rows of down, is read from global memory in fragment form (16 bytes per
//       lane), as sdnq_hip_lowrank_add reads up.  The MFMA is C^T = down . im2col(x)^T: a lane's four accumulators are four consecutive rank
//       columns of one row of t (an 8-byte store).  Which (c, i, j) the k-th column is comes from a table of the chunk in LDS (each lane
//       divides for one column, every gather reads a broadcast entry): no integer division in the gather.  A tap outside the image, a
//       column at or past K and a position at or past M are zeros in LDS; nothing outside x is read.  The waves' float32 partial sums are
//       added in LDS in ascending wave order: no atomics, the same bits on every call.  One launch, no workspace.
//       Why the waves split K and not the positions: a first form -- 64 positions per workgroup, its 4 waves sharing every chunk between
//       two barriers -- had B OH OW / 64 workgroups walk all of K in 2.2 us per chunk (105 us at 320 channels, 128 x 128, rank 16; 375 us
//       at 1280 channels, 32 x 32): one latency chain per CU, most CUs idle on the small images.  This form: 33 and 34 us there.
//
//   sdnq_hip_conv_lowrank_grad   out = scale * g^T . im2col(x), the gradient of down: a product that reduces over the output positions.
//       As sdnq_hip_lowrank_grad: the positions are cut into slabs of CLG_SLAB -- a constant of this file -- a workgroup sums one
//       (64-column tile of K, slab) in float32, and with more than one slab the partials [slab][K][rank] are added in ascending order
//       by lowrank_grad_sum_kernel: no atomics, the same bits on every call.  The window of im2col(x) is gathered as above into an
//       image [k][position]; here the reduction runs along the position, so a lane's operand (8 consecutive positions of one k) is 16
//       contiguous bytes of it: a plain ds_read_b128, the 16-byte slot mc of row k at slot mc ^ (k % 8) (rows 8 apart collide: 2-way;
//       worked out by hand, not confirmed by a counter run).  g goes through lowrank_grad's LDS image and transposed reads unchanged.
//   Both gather 16 elements per thread and stage with 2-byte loads and issue the next stage's loads before the MFMAs of the current one;
//   otherwise untuned.  Measurements: tools/conv_lora_bench.py, profiles/conv_lora_bench.jsonl.
#include "lowrank_dev.h"

namespace {

constexpr int CLG_SLAB = 256;  // output positions per partial sum of sdnq_hip_conv_lowrank_grad (tests/conv_lora_util.py restates it)

struct ConvGeo {
    int C, H, W, KH, KW, SH, SW, PH, PW, DH, DW, OH, OW;
    int64_t M, K;  // B OH OW, C KH KW
};

// column k of im2col(x): {c H W, i d_h, j d_w} of k = (c KH + i) KW + j; x < 0: at or past K
__device__ __forceinline__ int4 clr_tap(const ConvGeo& p, int64_t k) {
    if (k >= p.K) return make_int4(-1, 0, 0, 0);
    const int kk = (int)k, kprod = p.KH * p.KW;
    const int c = kk / kprod, t = kk - c * kprod, i = t / p.KW, j = t - i * p.KW;
    return make_int4(c * p.H * p.W, i * p.DH, j * p.DW, 0);
}

// row m of im2col(x) (m < limit): the image's offset in x and the input coordinates of tap (0, 0)
struct ClrPos {
    int64_t xb;
    int ih0, iw0;
    bool ok;
};
__device__ __forceinline__ ClrPos clr_pos(const ConvGeo& p, int64_t m, int64_t limit) {
    ClrPos r;
    r.ok = m < limit;
    int64_t b = 0, l = 0;
    if (r.ok) divmod(m, (int64_t)p.OH * p.OW, b, l);
    const int oh = (int)l / p.OW, ow = (int)l - oh * p.OW;
    r.xb = b * ((int64_t)p.C * p.H * p.W);
    r.ih0 = oh * p.SH - p.PH;
    r.iw0 = ow * p.SW - p.PW;
    return r;
}

// this thread's 16 elements of a window of im2col(x), 64 columns wide: row `pos`, columns tab[first + 4 q]
__device__ __forceinline__ void clr_gather(const uint16_t* __restrict__ x, const ConvGeo& p, const ClrPos& pos, const int4* tab, int first,
                                           uint16_t (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int4 e = tab[first + 4 * q];
        const int ih = pos.ih0 + e.y, iw = pos.iw0 + e.z;
        const bool ok = pos.ok && e.x >= 0 && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        v[q] = ok ? x[pos.xb + e.x + (int64_t)ih * p.W + iw] : (uint16_t)0;
    }
}

// ---- t = im2col(x) . down^T -----------------------------------------------------------------------------------------------------------
// NRT: rank tiles of 16 (rank <= 16 NRT); NW: waves of the workgroup.  grid: blocks of 16 output positions.
// The launch is a latency chain -- table, gather, LDS, MFMA per K chunk, few output positions to spread over the chip (1024 at 32 x 32) --
// so the chunks of 64 columns go round the NW waves (chunk c to wave c % NW), every wave on an LDS image and a tap table of its own with no
// workgroup barrier in its loop (LDS runs a wave's instructions in order; the compiler is held to the program order by clr_wave_sync), and
// the waves' float32 partial sums are added in LDS in ascending wave order at the end: the same bits on every call.
__device__ __forceinline__ void clr_wave_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

template <int T_ID, int NRT, int NW>
__global__ __launch_bounds__(NW * 64) void conv_lowrank_down_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ down,
                                                                    uint16_t* __restrict__ t, ConvGeo p, int R) {
    constexpr bool IS_BF16 = T_ID == SDNQ_BF16;
    constexpr int KC = 64;  // columns of im2col(x) per chunk
    __shared__ __attribute__((aligned(16))) uint8_t imgs[NW][KC * 32];  // per wave [k][16 positions]: lrg_frag<1>'s image
    __shared__ int4 tabs[NW][KC];
    __shared__ v4f red[NRT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gq = lane >> 4, li = lane & 15;
    const int64_t m0 = (int64_t)blockIdx.x * 16;
    uint8_t* img = imgs[wave];
    int4* tab = tabs[wave];
    const ClrPos pos = clr_pos(p, m0 + li, p.M);  // the gather's row: position li of the block, columns gq + 4 q of the chunk
    uint16_t v[16];
    v4f acc[NRT];
#pragma unroll
    for (int r = 0; r < NRT; ++r) acc[r] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    const v4i zero = {0, 0, 0, 0};
    const int64_t step = (int64_t)NW * KC;
    int64_t k0 = (int64_t)wave * KC;  // (wave-uniform)
    if (k0 < p.K) {
        tab[lane] = clr_tap(p, k0 + lane);
        clr_wave_sync();
        clr_gather(x, p, pos, tab, gq, v);
    }
    for (; k0 < p.K; k0 += step) {
        clr_wave_sync();  // the previous chunk's fragments are read
#pragma unroll
        for (int q = 0; q < 16; ++q) *(uint16_t*)(img + (gq + 4 * q) * 32 + 2 * li) = v[q];
        const bool more = k0 + step < p.K;
        if (more) tab[lane] = clr_tap(p, k0 + step + lane);
        clr_wave_sync();
        if (more) clr_gather(x, p, pos, tab, gq, v);  // in flight under the MFMAs
#pragma unroll
        for (int s = 0; s < KC; s += 32) {
            const v4i fx = lrg_frag<1>(img, s, 0, lane);  // positions li, columns k0 + s + 8 gq .. + 7
            const int64_t kc = k0 + s + 8 * gq;           // K % 8 == 0: a chunk is inside the row of down or past it
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const int rr = 16 * r + li;
                const v4i fd = (rr < R && kc < p.K) ? *(const v4i*)(down + (int64_t)rr * p.K + kc) : zero;
                acc[r] = mfma16<IS_BF16>(fd, fx, acc[r]);
            }
        }
    }
    // ((wave 0 + wave 1) + wave 2) + ...: one round per wave
    for (int w = 0; w < NW; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < NRT; ++r) red[r][lane] = w == 0 ? acc[r] : red[r][lane] + acc[r];
        }
        __syncthreads();
    }
    // accumulator e of rank tile r: rank 16 r + 4 gq + e of position m0 + li; tile r is stored by wave r % NW
    const int64_t m = m0 + li;
    if (m < p.M) {
        for (int r = wave; r < NRT; r += NW) {
            const int r0 = 16 * r + 4 * gq;
            if (r0 < R) {  // rank % 8 == 0: the 4 columns are inside the row or past it
                const v4f a = red[r][lane];
                uint2 w;
                w.x = pack2<T_ID>(a[0], a[1]);
                w.y = pack2<T_ID>(a[2], a[3]);
                *(uint2*)(t + m * R + r0) = w;
            }
        }
    }
}

// ---- out = scale * g^T . im2col(x) ----------------------------------------------------------------------------------------------------
// grid (64-column tiles of K, slabs).  `direct`: one slab -- scale, round and store out [R][K]; otherwise the float32 partial goes to
// part [slab][K][R] (the layout of lowrank_grad_sum_kernel).
template <bool IS_BF16, int NRT>
__global__ __launch_bounds__(256) void conv_lowrank_grad_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ gt, ConvGeo p,
                                                                int R, float scale, void* __restrict__ out, int out_dtype,
                                                                float* __restrict__ part, int direct) {
    constexpr int ROWS = 64, BB = NRT * 32;        // positions per stage; bytes per LDS row of g
    constexpr int BCH = NRT * 2;                   // 16-byte chunks per row of g
    constexpr int NB = (ROWS * BCH + 255) / 256;   // chunks of g per thread and stage
    __shared__ __attribute__((aligned(16))) uint8_t img_a[64 * 128];  // [k][position], the 16-byte slot mc of row k at mc ^ (k % 8)
    __shared__ __attribute__((aligned(16))) uint8_t img_b[ROWS * BB];
    __shared__ int4 tab[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gq = lane >> 4, li = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    const int64_t i_begin = (int64_t)blockIdx.y * CLG_SLAB;
    const int64_t i_end = i_begin + CLG_SLAB < p.M ? i_begin + CLG_SLAB : p.M;
    const v4i zero = {0, 0, 0, 0};
    if (tid < 64) tab[tid] = clr_tap(p, j0 + tid);
    __syncthreads();
    uint16_t v[16];
    v4i rb[NB];
    auto fetch = [&](int64_t i0) {
        clr_gather(x, p, clr_pos(p, i0 + lane, i_end), tab, wave, v);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int ch = tid + 256 * n, row = ch / BCH, col = (ch % BCH) * 8;
            const int64_t i = i0 + row;
            rb[n] = (ch < ROWS * BCH && i < i_end && col < R) ? *(const v4i*)(gt + i * R + col) : zero;  // rank % 8 == 0
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int kk = wave + 4 * q;
            *(uint16_t*)(img_a + kk * 128 + (((lane >> 3) ^ (kk & 7)) << 4) + 2 * (lane & 7)) = v[q];
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int ch = tid + 256 * n, row = ch / BCH, c8 = ch % BCH;
            if (ch < ROWS * BCH) *(v4i*)(img_b + row * BB + (((c8 >> 1) ^ lrg_swz<NRT>(row)) << 5) + ((c8 & 1) << 4)) = rb[n];
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
        const int kk = 16 * wave + li;            // this lane's column of the tile
#pragma unroll
        for (int s = 0; s < ROWS; s += 32) {
            const v4i fx = *(const v4i*)(img_a + kk * 128 + ((((s >> 3) + gq) ^ (kk & 7)) << 4));  // positions s + 8 gq .. + 7
#pragma unroll
            for (int r = 0; r < NRT; ++r) acc[r] = mfma16<IS_BF16>(fx, lrg_frag<NRT>(img_b, s, r, lane), acc[r]);
        }
    }
    // accumulator e of rank tile r: column j = j0 + 16 wave + 4 gq + e of im2col(x), rank 16 r + li
    const int64_t jb = j0 + 16 * wave + 4 * gq;
#pragma unroll
    for (int r = 0; r < NRT; ++r) {
        const int rr = 16 * r + li;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = jb + e;
            if (j < p.K && rr < R) {
                if (direct) st_rt(out, (int64_t)rr * p.K + j, scale * acc[r][e], out_dtype);
                else part[((int64_t)blockIdx.y * p.K + j) * R + rr] = acc[r][e];
            }
        }
    }
}

// the checks both entry points share; fills p
int clr_geometry(ConvGeo& p, int batch, int channels, int height, int width, int kh, int kw, int stride_h, int stride_w, int pad_h,
                 int pad_w, int dil_h, int dil_w, int rank) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || kh <= 0 || kw <= 0 || stride_h <= 0 || stride_w <= 0 || pad_h < 0 ||
        pad_w < 0 || dil_h <= 0 || dil_w <= 0 || rank < 8 || rank > 256 || (rank % 8) != 0)
        return SDNQ_ERR_SHAPE;
    const int64_t span_h = (int64_t)height + 2 * (int64_t)pad_h - (int64_t)dil_h * (kh - 1) - 1;
    const int64_t span_w = (int64_t)width + 2 * (int64_t)pad_w - (int64_t)dil_w * (kw - 1) - 1;
    if (span_h < 0 || span_w < 0) return SDNQ_ERR_SHAPE;  // the output would be empty
    const int64_t oh = span_h / stride_h + 1, ow = span_w / stride_w + 1;
    const int64_t k = (int64_t)channels * kh * kw, image = (int64_t)channels * height * width;
    // the gather's offsets inside one image, the tap offsets and the positions of one image are 32-bit
    if ((k % 8) != 0 || k > 0x7fffffff || image > 0x7fffffff || oh * ow > 0x7fffffff || (int64_t)dil_h * (kh - 1) > 0x3fffffff ||
        (int64_t)dil_w * (kw - 1) > 0x3fffffff || pad_h > 0x3fffffff || pad_w > 0x3fffffff || oh * stride_h > 0x3fffffff || ow * stride_w > 0x3fffffff)
        return SDNQ_ERR_SHAPE;
    p.C = channels; p.H = height; p.W = width; p.KH = kh; p.KW = kw; p.SH = stride_h; p.SW = stride_w; p.PH = pad_h; p.PW = pad_w;
    p.DH = dil_h; p.DW = dil_w; p.OH = (int)oh; p.OW = (int)ow;
    p.M = (int64_t)batch * oh * ow;
    p.K = k;
    return SDNQ_OK;
}

}  // namespace

extern "C" int sdnq_hip_conv_lowrank_down(const void* x, int dtype, int batch, int channels, int height, int width, int kh, int kw,
                                          int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, const void* down, int rank,
                                          void* t, sdnq_stream_t stream) {
    if (!x || !down || !t) return SDNQ_ERR_NULL;
    if (dtype != SDNQ_BF16 && dtype != SDNQ_F16) return SDNQ_ERR_DTYPE;
    ConvGeo p{};
    const int st = clr_geometry(p, batch, channels, height, width, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, rank);
    if (st != SDNQ_OK) return st;
    if (((uintptr_t)x % 16) || ((uintptr_t)down % 16) || ((uintptr_t)t % 16)) return SDNQ_ERR_ALIGN;
    const int64_t gx = (p.M + 15) / 16;
    if (gx > 0x7fffffff) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto kern, int waves) {
        hipLaunchKernelGGL(kern, grid, dim3(64 * waves), 0, s, (const uint16_t*)x, (const uint16_t*)down, (uint16_t*)t, p, rank);
    };
    // 16 waves share K up to rank 64; the wider accumulators of ranks beyond leave registers for 4 waves' worth of threads only
    const bool bf = dtype == SDNQ_BF16;
    if (rank <= 16) { if (bf) launch(conv_lowrank_down_kernel<SDNQ_BF16, 1, 16>, 16); else launch(conv_lowrank_down_kernel<SDNQ_F16, 1, 16>, 16); }
    else if (rank <= 32) { if (bf) launch(conv_lowrank_down_kernel<SDNQ_BF16, 2, 16>, 16); else launch(conv_lowrank_down_kernel<SDNQ_F16, 2, 16>, 16); }
    else if (rank <= 64) { if (bf) launch(conv_lowrank_down_kernel<SDNQ_BF16, 4, 16>, 16); else launch(conv_lowrank_down_kernel<SDNQ_F16, 4, 16>, 16); }
    else if (rank <= 128) { if (bf) launch(conv_lowrank_down_kernel<SDNQ_BF16, 8, 4>, 4); else launch(conv_lowrank_down_kernel<SDNQ_F16, 8, 4>, 4); }
    else { if (bf) launch(conv_lowrank_down_kernel<SDNQ_BF16, 16, 4>, 4); else launch(conv_lowrank_down_kernel<SDNQ_F16, 16, 4>, 4); }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int64_t sdnq_hip_conv_lowrank_grad_workspace_bytes(int batch, int channels, int height, int width, int kh, int kw, int stride_h,
                                                              int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int rank) {
    ConvGeo p{};
    const int st = clr_geometry(p, batch, channels, height, width, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, rank);
    if (st != SDNQ_OK) return st;
    const int64_t slabs = (p.M + CLG_SLAB - 1) / CLG_SLAB;
    return slabs <= 1 ? 0 : slabs * p.K * rank * 4;
}

extern "C" int sdnq_hip_conv_lowrank_grad(const void* x, int dtype, int batch, int channels, int height, int width, int kh, int kw,
                                          int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, const void* g, int rank,
                                          float scale, void* out, int out_dtype, void* workspace, int64_t workspace_bytes,
                                          sdnq_stream_t stream) {
    if (!x || !g || !out) return SDNQ_ERR_NULL;
    if ((dtype != SDNQ_BF16 && dtype != SDNQ_F16) || out_dtype < 0 || out_dtype > 2) return SDNQ_ERR_DTYPE;
    ConvGeo p{};
    const int st = clr_geometry(p, batch, channels, height, width, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, rank);
    if (st != SDNQ_OK) return st;
    if (((uintptr_t)x % 16) || ((uintptr_t)g % 16) || ((uintptr_t)out % 16)) return SDNQ_ERR_ALIGN;
    const int64_t slabs = (p.M + CLG_SLAB - 1) / CLG_SLAB;
    const int64_t need = slabs <= 1 ? 0 : slabs * p.K * rank * 4;
    if (need > 0) {
        if (!workspace) return SDNQ_ERR_NULL;
        if (workspace_bytes < need) return SDNQ_ERR_SHAPE;
        if ((uintptr_t)workspace % 16) return SDNQ_ERR_ALIGN;
    }
    const int64_t gx = (p.K + 63) / 64, total = p.K * rank;
    if (slabs > 65535 || (total + 255) / 256 > 0x7fffffff) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)slabs), block(256);
    hipStream_t s = (hipStream_t)stream;
    const int direct = slabs == 1;
    float* part = (float*)workspace;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, (const uint16_t*)x, (const uint16_t*)g, p, rank, scale, out, out_dtype, part, direct);
    };
    const bool bf = dtype == SDNQ_BF16;
    if (rank <= 16) { if (bf) launch(conv_lowrank_grad_kernel<true, 1>); else launch(conv_lowrank_grad_kernel<false, 1>); }
    else if (rank <= 32) { if (bf) launch(conv_lowrank_grad_kernel<true, 2>); else launch(conv_lowrank_grad_kernel<false, 2>); }
    else if (rank <= 64) { if (bf) launch(conv_lowrank_grad_kernel<true, 4>); else launch(conv_lowrank_grad_kernel<false, 4>); }
    else if (rank <= 128) { if (bf) launch(conv_lowrank_grad_kernel<true, 8>); else launch(conv_lowrank_grad_kernel<false, 8>); }
    else { if (bf) launch(conv_lowrank_grad_kernel<true, 16>); else launch(conv_lowrank_grad_kernel<false, 16>); }
    SDNQ_CHECK_LAUNCH();
    if (!direct) {
        hipLaunchKernelGGL(lowrank_grad_sum_kernel, dim3((unsigned)((total + 255) / 256)), block, 0, s, (const float*)part, slabs, p.K, rank,
                           scale, 1, out, out_dtype);
        SDNQ_CHECK_LAUNCH();
    }
    return SDNQ_OK;
}
