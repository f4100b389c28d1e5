// Transposed convolutions on gfx950 as GEMM + col2im: the weight-side and output-side kernels of SDNQConvTranspose1d / 2d / 3d.
//
//   quantized_conv_transpose_{1,2,3}d_forward (layers/conv/forward.py:85-99): F.conv_transposeNd(x, dequantize(W), bias, stride, padding,
//   output_padding, groups, dilation) with W [C_in][C_out / groups][k...].  Per conv group g that is
//       cols[(b, l)][(co, kpos)] = sum_ci x[b][ci][l] * W[ci][co][kpos]      (M = B * L input positions, K = C_in / groups, N = P = C_out / groups * prod(k))
//   -- the float GEMM of linear_float.hip with a float32 store -- and every output element then gathers the taps that reach it.
//
//   sdnq_hip_dequant_convt  <- SDNQDequantizer.__call__ on a transposed-conv weight (dequantizer.py:63-84), written straight into the GEMM's
//       weight operand [groups][P][C_in / groups] (K contiguous).  A workgroup takes a 64 (ci) x 64 (column) tile of the stored [C_in][P]
//       matrix: thread t decodes the 16 codes (row t / 4, chunk t % 4) with load16_values (weight_dev.h / unpack_dev.h; one 16-byte load
//       for 8-bit codes), applies scale / zero point with the arithmetic of dequant16 -- the product or fma in float32, rounded to the
//       scale dtype when that is a 16-bit one -- and writes the values transposed into LDS; the tile leaves as 16-byte runs along ci.
//       Coalesced 16-byte accesses are the code loads and the stores only: scale and zero point are read one float per element (every
//       lane its own 16, although the rows of a tile share them in the column layout; they hit L1 / L2 after the first row) -- untuned.
//       Two scale layouts (quantizer.py:129-133, 210-214): one scale per column [1][P] (reduction over C_in), or the square grouped layout
//       [C_in][1][num_groups][k...] in which column (co, kpos) of row ci takes scale[ci][co % num_groups][kpos] -- the index is the flat column
//       modulo num_groups * prod(k) either way (modulo P for the column layout, with no row offset).
//
//   sdnq_hip_col2im  <- the scatter half of conv_transposeNd, in gather form: one thread owns one output element (b, co, od, oh, ow) and adds,
//       in float32 and in the fixed order kd, kh, kw ascending, the taps with (o + pad - k * dil) % stride == 0 whose quotient is inside the
//       input; starts from bias[co]; one rounding at the store.  No atomics: the same bits on every call.
//       Thread mapping: a workgroup computes 16 channels x 16 consecutive output positions of one image; in the compute phase consecutive
//       lanes are consecutive CHANNELS (lane % 16) of one output position, so for every tap a wave's loads lie in at most 4 rows of cols (its 4
//       output positions), 16 lanes per row at a stride of prod(k) floats (4-byte loads, not coalesced: untuned); the results cross a
//       16 x 16 LDS tile and leave with consecutive lanes on consecutive output positions (32- / 64-byte runs of the NC(D)HW output).
//       blockIdx.x = image * tiles + tile of 16 output positions, blockIdx.y = tile of 16 channels: no limit on the batch but the grid's 2^31.
#include "weight_dev.h"

namespace {

struct ConvtDeq {
    const void* w;
    const float* scale;
    const float* zp;
    int64_t c_in, P, kg;  // stored weight [c_in][P]; kg = C_in / groups
    int period;           // scale index of column k: k % period
    int row_stride;       // scales per row ci: 0 (one scale per column) or period (square grouped layout)
    int sdt;              // SdnqWeight.scale_dtype
    WeightFmt fmt;
};

template <int T_ID>
__global__ __launch_bounds__(256) void dequant_convt_kernel(ConvtDeq p, void* __restrict__ out) {
    constexpr int VN = Vec16<T_ID>::n, CH = 64 / VN;
    __shared__ float tile[64][65];  // [column][ci]
    const int tid = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    {
        const int r = tid >> 2, ch = tid & 3;
        const int64_t ci = c0 + r, k = k0 + ch * 16;
        if (ci < p.c_in && k < p.P) {  // P % 16 == 0: a run of 16 never leaves its row
            float v[16];
            load16_values(p.w, ci * p.P + k, p.fmt, v);
            const float* srow = p.scale + ci * p.row_stride;
            const float* zrow = p.zp ? p.zp + ci * p.row_stride : nullptr;
            int s = (int)(k % p.period);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                v[j] = zrow ? fmaf(v[j], srow[s], zrow[s]) : v[j] * srow[s];  // torch.addcmul == single-rounding fma
                if (++s == p.period) s = 0;
            }
            if (p.sdt != SDNQ_F32) {  // 16-bit scale / zero_point: the product is rounded ONCE to that dtype (dequantizer.py:27, 63)
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = round_rt(v[j], p.sdt);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) tile[ch * 16 + j][r] = v[j];
        }
    }
    __syncthreads();
    for (int o = tid; o < 64 * CH; o += 256) {
        const int kl = o / CH, cc = (o % CH) * VN;
        const int64_t k = k0 + kl, ci = c0 + cc;
        if (k < p.P && ci < p.c_in) {  // kg % 16 == 0: a run of VN channels stays inside one conv group, 16-byte aligned
            const int64_t g = ci / p.kg, cig = ci - g * p.kg;
            float f[VN];
#pragma unroll
            for (int e = 0; e < VN; ++e) f[e] = tile[kl][cc + e];
            *(uint4*)((uint8_t*)out + ((g * p.P + k) * p.kg + cig) * FT<T_ID>::bytes) = Vec16<T_ID>::pack(f);
        }
    }
}

struct Col2imParams {
    const float* cols;
    const void* bias;
    void* out;
    int64_t ldcols;
    int C, D, H, W, OD, OH, OW;
    int tiles;  // tiles of 16 output positions per image
    int KD, KH, KW, SD, SH, SW, PD, PH, PW, DD, DH, DW;
};

template <int T_ID>
__global__ __launch_bounds__(256) void col2im_kernel(Col2imParams a) {
    __shared__ float tile[16][17];  // [channel][output position]
    const int tid = threadIdx.x;
    const int64_t osz = (int64_t)a.OD * a.OH * a.OW;
    const int b = (int)(blockIdx.x / (unsigned)a.tiles);
    const int64_t o0 = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)a.tiles) * 16;
    const int c0 = blockIdx.y * 16;
    {
        const int co = c0 + (tid & 15);
        const int64_t o = o0 + (tid >> 4);
        if (co < a.C && o < osz) {
            const int ow = (int)(o % a.OW);
            const int64_t t = o / a.OW;
            const int oh = (int)(t % a.OH), od = (int)(t / a.OH);
            float acc = a.bias ? FT<T_ID>::load(a.bias, co) : 0.0f;
            const float* cbase = a.cols + (int64_t)co * (a.KD * a.KH * a.KW);
            for (int kd = 0; kd < a.KD; ++kd) {
                const int td = od + a.PD - kd * a.DD;
                if (td < 0 || td % a.SD) continue;
                const int id = td / a.SD;
                if (id >= a.D) continue;
                for (int kh = 0; kh < a.KH; ++kh) {
                    const int th = oh + a.PH - kh * a.DH;
                    if (th < 0 || th % a.SH) continue;
                    const int ih = th / a.SH;
                    if (ih >= a.H) continue;
                    const int64_t row0 = (((int64_t)b * a.D + id) * a.H + ih) * a.W;
                    for (int kw = 0; kw < a.KW; ++kw) {
                        const int tw = ow + a.PW - kw * a.DW;
                        if (tw < 0 || tw % a.SW) continue;
                        const int iw = tw / a.SW;
                        if (iw >= a.W) continue;
                        acc += cbase[(row0 + iw) * a.ldcols + ((kd * a.KH + kh) * a.KW + kw)];
                    }
                }
            }
            tile[tid & 15][tid >> 4] = acc;
        }
    }
    __syncthreads();
    {
        const int co = c0 + (tid >> 4);
        const int64_t o = o0 + (tid & 15);
        if (co < a.C && o < osz) FT<T_ID>::store(a.out, ((int64_t)b * a.C + co) * osz + o, tile[tid >> 4][tid & 15]);
    }
}

}  // namespace

extern "C" int sdnq_hip_dequant_convt(const SdnqWeight* w, int groups, int scale_groups, void* out, int out_dtype, sdnq_stream_t stream) {
    if (!w || !out) return SDNQ_ERR_NULL;
    if (out_dtype < 0 || out_dtype > 2) return SDNQ_ERR_DTYPE;
    if (w->kind == SDNQ_KIND_CODEBOOK || w->svd_up || w->svd_down) return SDNQ_ERR_UNSUPPORTED;
    const int kprod = w->positions > 1 ? w->positions : 1;
    // the format checks of every weight-side entry point, on the flat [C_in][P] view
    SdnqWeight flat = *w;
    flat.positions = 1;
    flat.group_size = w->k;
    DeqParams dp;
    const int st = fill_params(&flat, dp);
    if (st != SDNQ_OK) return st;
    const int64_t c_in = w->n, P = w->k;
    if (groups <= 0 || c_in % groups || ((c_in / groups) % 16) != 0 || (P % kprod) != 0) return SDNQ_ERR_SHAPE;
    if (scale_groups < 0 || (scale_groups > 1 && ((P / kprod) % scale_groups) != 0)) return SDNQ_ERR_SHAPE;
    if ((uintptr_t)out % 16) return SDNQ_ERR_ALIGN;
    ConvtDeq p;
    p.w = dp.w; p.scale = dp.scale; p.zp = dp.zp; p.c_in = c_in; p.P = P; p.kg = c_in / groups; p.sdt = dp.sdt; p.fmt = dp.fmt;
    if (scale_groups > 1) {
        p.period = scale_groups * kprod;
        p.row_stride = p.period;
    } else {
        if (P > 0x7fffffff) return SDNQ_ERR_SHAPE;
        p.period = (int)P;
        p.row_stride = 0;
    }
    const int64_t gx = (P + 63) / 64, gy = (c_in + 63) / 64;
    if (gx > 0x7fffffff || gy > 65535) return SDNQ_ERR_SHAPE;
    dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (out_dtype) {
        case SDNQ_F32: hipLaunchKernelGGL(dequant_convt_kernel<SDNQ_F32>, grid, block, 0, s, p, out); break;
        case SDNQ_BF16: hipLaunchKernelGGL(dequant_convt_kernel<SDNQ_BF16>, grid, block, 0, s, p, out); break;
        default: hipLaunchKernelGGL(dequant_convt_kernel<SDNQ_F16>, grid, block, 0, s, p, out); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_col2im(const float* cols, int64_t ldcols, const void* bias, int dtype, void* out, int batch, int channels,
                               int in_d, int in_h, int in_w, int out_d, int out_h, int out_w, int kd, int kh, int kw, int stride_d,
                               int stride_h, int stride_w, int pad_d, int pad_h, int pad_w, int dil_d, int dil_h, int dil_w,
                               sdnq_stream_t stream) {
    if (!cols || !out) return SDNQ_ERR_NULL;
    if (dtype < 0 || dtype > 2) return SDNQ_ERR_DTYPE;
    if (batch <= 0 || channels <= 0 || in_d <= 0 || in_h <= 0 || in_w <= 0 || out_d <= 0 || out_h <= 0 || out_w <= 0 || kd <= 0 || kh <= 0 ||
        kw <= 0 || stride_d <= 0 || stride_h <= 0 || stride_w <= 0 || pad_d < 0 || pad_h < 0 || pad_w < 0 || dil_d <= 0 || dil_h <= 0 || dil_w <= 0)
        return SDNQ_ERR_SHAPE;
    const int64_t kprod = (int64_t)kd * kh * kw;
    if (kprod > 0x7fffffff / channels || ldcols < (int64_t)channels * kprod) return SDNQ_ERR_SHAPE;
    // every tap's input index is checked against the input extent in the kernel, so no output extent can make it read outside cols;
    // an extent beyond what the geometry reaches with output_padding < max(stride, dilation) is a caller's mistake all the same
    const int in[3] = {in_d, in_h, in_w}, on[3] = {out_d, out_h, out_w}, kk[3] = {kd, kh, kw}, ss[3] = {stride_d, stride_h, stride_w},
              pp[3] = {pad_d, pad_h, pad_w}, dd[3] = {dil_d, dil_h, dil_w};
    for (int i = 0; i < 3; ++i) {
        const int64_t base = (int64_t)(in[i] - 1) * ss[i] - 2 * (int64_t)pp[i] + (int64_t)dd[i] * (kk[i] - 1) + 1;
        if (on[i] < base || on[i] >= base + (ss[i] > dd[i] ? ss[i] : dd[i])) return SDNQ_ERR_SHAPE;
    }
    if ((uintptr_t)cols % 4) return SDNQ_ERR_ALIGN;
    const int64_t osz = (int64_t)out_d * out_h * out_w, tiles = (osz + 15) / 16;
    if (tiles > 0x7fffffff / batch || (channels + 15) / 16 > 65535) return SDNQ_ERR_SHAPE;
    const int64_t gx = tiles * batch;
    Col2imParams a;
    a.cols = cols; a.bias = bias; a.out = out; a.ldcols = ldcols; a.C = channels; a.tiles = (int)tiles;
    a.D = in_d; a.H = in_h; a.W = in_w; a.OD = out_d; a.OH = out_h; a.OW = out_w; a.KD = kd; a.KH = kh; a.KW = kw;
    a.SD = stride_d; a.SH = stride_h; a.SW = stride_w; a.PD = pad_d; a.PH = pad_h; a.PW = pad_w; a.DD = dil_d; a.DH = dil_h; a.DW = dil_w;
    dim3 grid((unsigned)gx, (unsigned)((channels + 15) / 16)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case SDNQ_F32: hipLaunchKernelGGL(col2im_kernel<SDNQ_F32>, grid, block, 0, s, a); break;
        case SDNQ_BF16: hipLaunchKernelGGL(col2im_kernel<SDNQ_BF16>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(col2im_kernel<SDNQ_F16>, grid, block, 0, s, a); break;
    }
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}
