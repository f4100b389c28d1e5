// How wide is the adder inside the floating-point MFMAs of the GEMMs (32x32) and of lowrank_down (16x16x32)?  One wave, one instruction per case, no library kernel.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/micro/mfma_sum_probe.hip -o /tmp/mfma_sum_probe && /tmp/mfma_sum_probe
//
// D = C + sum_k a_k * b_k.  With C = 2^s and products equal to 1 the exact D is an integer, and D is compared with that integer (in
// double).  fp32 holds it for s <= 23 (2^24 + 1 is not a float, so s = 24 always fails (a): the probe's ceiling is 23); below that a
// wrong D means that the instruction dropped bits of a product that lies s binary places below its largest addend:
//   (a) one product equal to 1, in the first K slot and, separately, in the last one;      D = 2^s + 1
//   (b) every product of the K equal to 1;                                                 D = 2^s + K
// The largest s for which every element of every (a) and (b) case is exact is the "span" the exact-sum tests rely on
// (tests/exact_inputs.py takes its budget from the recorded output, profiles/mfma_sum_probe.txt).
//   (c) for information: C = 0, one product equal to 2^s beside one product equal to 1 (the spread between two products of ONE
//       instruction; e4m3 reaches 2^8 per operand, so s <= 16 there).                      D = 2^s + 1
// Both operands use the same lane -> K mapping (lane / 32 picks the K half -- lane / 16 the K quarter of the 16x16x32 instructions --,
// the register slot the element), so "slot j of lane group g"
// of A always meets the same slot of B: the probe needs no knowledge of the K order inside a lane.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

enum { FP8 = 0, BF16 = 1, F16 = 2, BF16_16 = 3, F16_16 = 4, N_INS = 5 };
static const char* const NAMES[N_INS] = {"v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3, unit scales)", "v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x16_f16",
                                         "v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16"};
static const int KDIM[N_INS] = {64, 16, 16, 32, 32};
static const int ELEM_BYTES[N_INS] = {1, 2, 2, 2, 2};
static const int GROUPS[N_INS] = {2, 2, 2, 4, 4};    // lane groups along K: 64 / GROUPS lanes each
static const int N_OUT[N_INS] = {1024, 1024, 1024, 256, 256};  // outputs of one instruction (64 lanes x 16 or x 4 accumulators)

// fragments: 32 bytes per lane for each operand (the 16-bit instructions read the first 16); out: 64 lanes x 16 accumulators (x 4: 16x16x32)
template <int INS> __global__ void __launch_bounds__(64) probe(const uint8_t* __restrict__ fa, const uint8_t* __restrict__ fb, float cval, float* __restrict__ out) {
    const int lane = threadIdx.x;
    if constexpr (INS == BF16_16 || INS == F16_16) {
        v4f c4 = {cval, cval, cval, cval};
        const v4i a = *(const v4i*)(fa + lane * 32), b = *(const v4i*)(fb + lane * 32);
        if constexpr (INS == BF16_16) c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c4, 0, 0, 0);
        else c4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c4, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[lane * 4 + i] = c4[i];
        return;
    }
    v16f c;
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = cval;
    if constexpr (INS == FP8) {
        const v8i a = *(const v8i*)(fa + lane * 32), b = *(const v8i*)(fb + lane * 32);
        c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    } else if constexpr (INS == BF16) {
        const v4i a = *(const v4i*)(fa + lane * 32), b = *(const v4i*)(fb + lane * 32);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    } else {
        const v4i a = *(const v4i*)(fa + lane * 32), b = *(const v4i*)(fb + lane * 32);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[lane * 16 + i] = c[i];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// the encoding of 2^p in each format (p within the normal range)
static unsigned pow2(int ins, int p) {
    if (ins == FP8) return (unsigned)(p + 7) << 3;
    if (ins == BF16 || ins == BF16_16) return (unsigned)(p + 127) << 7;
    return (unsigned)(p + 15) << 10;
}
struct Frag {
    std::vector<uint8_t> a, b;
    int ins;
    explicit Frag(int ins_) : a(64 * 32, 0), b(64 * 32, 0), ins(ins_) {}
    int slots() const { return KDIM[ins] / GROUPS[ins]; }  // K elements per lane
    void set(int group, int slot, unsigned ea, unsigned eb) {  // the same (group, slot) in all 32 lanes of the group
        const int gl = 64 / GROUPS[ins];
        for (int l = 0; l < gl; ++l) {
            const size_t off = (size_t)(group * gl + l) * 32 + (size_t)slot * ELEM_BYTES[ins];
            memcpy(&a[off], &ea, ELEM_BYTES[ins]);
            memcpy(&b[off], &eb, ELEM_BYTES[ins]);
        }
    }
};

static uint8_t *d_a, *d_b;
static float* d_out;
// runs one instruction; returns the number of its outputs (1024, or 256 of a 16x16x32 instruction) that differ from `want`, and the first such output
static int run(const Frag& f, float cval, double want, float* first_bad) {
    float h[1024];
    if (hipMemcpy(d_a, f.a.data(), 2048, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_b, f.b.data(), 2048, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (f.ins == FP8) hipLaunchKernelGGL(probe<FP8>, dim3(1), dim3(64), 0, 0, d_a, d_b, cval, d_out);
    else if (f.ins == BF16) hipLaunchKernelGGL(probe<BF16>, dim3(1), dim3(64), 0, 0, d_a, d_b, cval, d_out);
    else if (f.ins == F16) hipLaunchKernelGGL(probe<F16>, dim3(1), dim3(64), 0, 0, d_a, d_b, cval, d_out);
    else if (f.ins == BF16_16) hipLaunchKernelGGL(probe<BF16_16>, dim3(1), dim3(64), 0, 0, d_a, d_b, cval, d_out);
    else hipLaunchKernelGGL(probe<F16_16>, dim3(1), dim3(64), 0, 0, d_a, d_b, cval, d_out);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d_out, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int bad = 0;
    for (int i = 0; i < N_OUT[f.ins]; ++i)
        if ((double)h[i] != want) { if (!bad) *first_bad = h[i]; ++bad; }
    return bad;
}

int main() {
    CHECK(hipMalloc(&d_a, 2048)); CHECK(hipMalloc(&d_b, 2048)); CHECK(hipMalloc(&d_out, 1024 * sizeof(float)));
    for (int ins = 0; ins < N_INS; ++ins) {
        const int K = KDIM[ins];
        const unsigned one = pow2(ins, 0);
        printf("%s  K = %d\n", NAMES[ins], K);
        int span = 0, span_c = 0;
        bool open = true, open_c = true;
        const int c_max = ins == FP8 ? 16 : 24;
        for (int s = 1; s <= 24; ++s) {
            const float big = (float)(1u << s);
            float got[4] = {0, 0, 0, 0};
            int bad[4] = {0, 0, 0, 0};
            Frag first(ins), last(ins), full(ins), two(ins);
            first.set(0, 0, one, one);
            last.set(GROUPS[ins] - 1, last.slots() - 1, one, one);
            for (int g = 0; g < GROUPS[ins]; ++g) for (int j = 0; j < full.slots(); ++j) full.set(g, j, one, one);
            bad[0] = run(first, big, (double)big + 1.0, &got[0]);
            bad[1] = run(last, big, (double)big + 1.0, &got[1]);
            bad[2] = run(full, big, (double)big + K, &got[2]);
            if (s <= c_max) {
                two.set(0, 0, one, one);
                two.set(1, 1, pow2(ins, (s + 1) / 2), pow2(ins, s / 2));
                bad[3] = run(two, 0.0f, (double)big + 1.0, &got[3]);
            }
            if (bad[0] < 0 || bad[1] < 0 || bad[2] < 0 || bad[3] < 0) { printf("HIP error during s = %d\n", s); return 2; }
            const bool ok = !bad[0] && !bad[1] && !bad[2];
            if (open && ok) span = s; else open = false;
            if (s <= c_max) { if (open_c && !bad[3]) span_c = s; else open_c = false; }
            printf("  s=%2d  (a) first slot %-5s  (a) last slot %-5s  (b) full K %-5s", s, bad[0] ? "WRONG" : "exact", bad[1] ? "WRONG" : "exact", bad[2] ? "WRONG" : "exact");
            if (s <= c_max) printf("  (c) two products %-5s", bad[3] ? "WRONG" : "exact");
            if (bad[0]) printf("  [a-first: %d of %d wrong, e.g. D - 2^s = %g]", bad[0], N_OUT[ins], (double)got[0] - (double)big);
            if (bad[1]) printf("  [a-last: %d wrong, D - 2^s = %g]", bad[1], (double)got[1] - (double)big);
            if (bad[2]) printf("  [b: %d wrong, D - 2^s = %g]", bad[2], (double)got[2] - (double)big);
            if (bad[3]) printf("  [c: %d wrong, D - 2^s = %g]", bad[3], (double)got[3] - (double)big);
            printf("\n");
        }
        printf("  measured span, accumulator against products (a, b): %d bits\n", span);
        printf("  for information, product against product (c): exact up to s = %d of the %d the format allows\n\n", span_c, c_max);
    }
    CHECK(hipFree(d_a)); CHECK(hipFree(d_b)); CHECK(hipFree(d_out));
    return 0;
}
