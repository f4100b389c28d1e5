// The w8a8 Linear as ONE launch: the GEMM workgroup row-quantizes its own activation rows into LDS (north_star: "activations
// row-quantized on the fly in LDS") and streams only the weight operand through its LDS-DMA ring.
//
// Reference chain replaced (linear_int8.py:15-22, 64 -> kernels/triton_scaled_mm.py:194-232; linear_fp8.py the same with e4m3fn codes):
//   x.to(float32); scale = amax(|x|, -1) / 127; q = clamp(round(x / scale), -128, 127).to(int8)      one Inductor kernel per call
//   out = (f32(q @ Wq^T) * scale) * ws [+ bias]                                                        the Triton scaled-mm kernel
// Here (rounds 1-4): sdnq_hip_rowquant + sdnq_hip_scaled_mm, two launches -- at the bs = 1 sizes of an SDXL step the first is 5 us of
// launch boundary, cold first bytes and a write-through of codes that the second launch waits another 1.5 us to read back.
//
// Why this form and not the ones measured before (profiles/r02_fused_rowquant_prologue.txt, r02_sync_lab.txt):
//   * the row scale needs the WHOLE row, so a workgroup quantizes whole rows: BM = 64 rows x K <= 1280 codes = 80 KB stay RESIDENT in
//     LDS (in the ring's own stage layout: 128-byte rows, XOR-swizzled chunks), next to a 4-deep ring of weight stages (64 KB);
//   * every workgroup of a row block repeats the quantization (tiles_n of them: 10 for N = 1280) -- affordable only since round 4's
//     lean arithmetic (quant8_dev.h: ~3 instructions per element instead of ~20; round 2 measured this form at 17.9 us with the
//     IEEE-division sequence);
//   * the K loop then fills LDS with weight rows only (2/3 of the bytes per stage of the 64x128 tile), and nothing is exchanged
//     between workgroups: no flags, no grid barrier, no deadlock to argue about.
// Bit-identical to the two-launch route by construction (the same quant8, the same MFMA, the same epilogue expression) and by
// tests/test_gemm_aq.py; tests/test_gemm_aq_geometry.py runs the same cases on each tile geometry below.
//
// The 32 x 256 tile runs WAVE-PRIVATE weight slabs (SLAB in the kernel): its waves are laid out 1 x 8, so every wave multiplies the same
// 32 activation rows by its own 32 weight rows and no weight byte is read by two waves -- the ring is a landing place only.  There a
// wave moves its own rows (four pieces of every stage), all three ring slots are in flight behind the rows, and a stage is drained by
// its wave alone: counted vmcnt for its own pieces, fragments into registers, the slot refilled with stage j + 3 at once.  Two stages
// are drained under the quantization, the others in a K loop without a barrier, in the ring form's order of stages and sub-steps: the
// same bits (tests/test_gemm_aq_regslab.py: a placement census of every weight byte, every stage count and edge).  Draining ALL stages
// into registers under the quantization (160 registers per lane; built and measured) lost: the MFMAs then start only when the last
// weight byte has landed.  Where the caller holds the fragment-ordered copy of an int8 weight
// (sdnq_hip_linear_w8a8_fused_slab), the tile runs its DIRECT form instead: no ring, the fragments loaded from the copy straight into a
// three-stage ring of registers (DIRECT in the kernel; tests/test_gemm_aq_direct.py).
//
// Quantization layout (64 x 128 tile; the 32 x 256 tile: rows 4w .. 4w+3, one pass): wave w owns tile rows 8w .. 8w+7 in two passes of 4 rows; a row is read by a QUARTER wave (16 lanes x 16 bytes
// = 128 elements per load instruction = one K stage), so the row amax is a reduction inside one 16-lane DPP row (four DPP exchanges,
// no LDS) and lane l's j-th chunk (8 elements) IS bytes 8 (l & 15) .. +8 of stage j's row: one ds_write_b64.
#include "gemm_dev.h"
#include "quant8_dev.h"

namespace {

// Tile geometries (template parameters BM x BN of the kernel and its ring depth; BK, the wave count and the 32x32 MFMA are common):
//   0: 64 x 128, 4 ring slots : waves 2 x 4; a wave quantizes 8 rows in two passes; 16-KB weight stages; tiles_n workgroups repeat a row block
//   1: 32 x 256, 3 ring slots : waves 1 x 8; a wave quantizes 4 rows in one pass (half the ingest and the arithmetic in front of the K loop,
//                               half the redundancy across a row block); 32-KB weight stages, 40 + 96 KB of LDS at K = 1280; every wave
//                               moves and drains its own weight rows, no barrier in the K loop (the slab form: BN / 32 == NW)
// and the "tall" form for K <= 640 (five stages held) where the 64 x 128 tiles of a problem outnumber the CUs:
//   2: 64 x 128, 2 ring slots : the tile of geometry 0 on a thin ring: 40 KB image + 32 KB ring, so TWO workgroups share a CU (the second
//                               one hides the first one's stage waits, as in the two-launch GEMM's 3 slots x 2 workgroups) and
//                               2 x CUs tiles are resident at once
// Every tile is one 32 x 32 accumulator per wave.  A 128 x 128 tile with two per wave (one workgroup per CU, half the tiles) was built
// for the tall problems and lost: 19 799 against 13 070 ticks per workgroup (profiles/linear_aq_k640_tall.txt).
constexpr int BK = 128, NW = 8, NT = NW * 64;

// The form geometry 1 runs in on int8 where the caller passes the slab copy of the weight (sdnq_hip_linear_w8a8_fused_slab): the direct
// form with AQ_DIRECT_STAGES register stages, or 0: the LDS ring (as without a copy).  Depths 3, 4, 6 and 8 were built and measured in
// the step: 3 and 4 level, 6 and 8 behind; 3 takes the fewest registers.
constexpr int AQ_DIRECT_STAGES = 3;

struct AqParams {
    const float* sb;      // [N] weight row scales
    const void* bias;     // [N] or null
    void* out;            // [M][ldc]
    int64_t ldc;
    int bias_dtype;
    const uint8_t* pf_ptr[4];  // weight prefetch hosted by this launch (sdnq_hip_prefetch_hint)
    int pf_lines[4];
    unsigned long long* trace;  // lab: per-workgroup phase stamps (8 per workgroup), or null
};

// The members of a GROUPED launch (layers that read one activation: sdnq_hip_linear_w8a8_fused_grouped), by value in the kernel arguments.
// Column block t of the launch belongs to member t / bpm and is that member's block t % bpm; the member's slab copy, scales and bias
// stand in for w, AqParams.sb and AqParams.bias, and its output is the contiguous [M][N] matrix at element offset M * N * member of
// AqParams.out (the layout of sdnq_hip_scaled_mm_grouped).
constexpr int AQ_GROUP_MAX = 8;
struct AqGroup {
    const uint8_t* slab[AQ_GROUP_MAX];
    const float* sb[AQ_GROUP_MAX];
    const void* bias[AQ_GROUP_MAX];
    int bpm;  // column blocks per member
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

template <int MM> struct AqMma;
template <> struct AqMma<SDNQ_MM_I8> {
    typedef v16i acc_t;
    typedef v4i frag_t;
    static constexpr int KB = 32;  // K bytes per MFMA
    static __device__ __forceinline__ frag_t load(const uint8_t* s, int r, int ks, int fgrp) {
        return *(const v4i*)(s + r * 128 + (((ks * 2 + fgrp) ^ ((r >> 1) & 7)) << 4));
    }
    static __device__ __forceinline__ void mma(acc_t& c, const frag_t& w, const frag_t& x) { c = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, x, c, 0, 0, 0); }
    static __device__ __forceinline__ float tof(const acc_t& c, int i) { return (float)c[i]; }
};
template <> struct AqMma<SDNQ_MM_FP8> {
    typedef v16f acc_t;
    typedef v8i frag_t;
    static constexpr int KB = 64;
    static __device__ __forceinline__ frag_t load(const uint8_t* s, int r, int ks, int fgrp) {
        const int sw = (r >> 1) & 7;
        const v4i lo = *(const v4i*)(s + r * 128 + (((ks * 4 + fgrp * 2) ^ sw) << 4));
        const v4i hi = *(const v4i*)(s + r * 128 + (((ks * 4 + fgrp * 2 + 1) ^ sw) << 4));
        return (v8i){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    static __device__ __forceinline__ void mma(acc_t& c, const frag_t& w, const frag_t& x) {
        c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w, x, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    }
    static __device__ __forceinline__ float tof(const acc_t& c, int i) { return c[i]; }
};

// The kernel's text lives in gemm_aq_kernel.h, included once per form: linear_aq_kernel (AQ_GROUPED 0; its text, and therefore its code,
// is what it was before the grouped form existed) and linear_aq_grouped_kernel (AQ_GROUPED 1: the direct form for several layers that
// read one activation, sdnq_hip_linear_w8a8_fused_grouped).  As one inlined function under two kernels the same text changed the
// register allocation of the existing instantiations (tools/compare_kernels.py).
#define AQ_GROUPED 0
#include "gemm_aq_kernel.h"
#undef AQ_GROUPED
#define AQ_GROUPED 1
#include "gemm_aq_kernel.h"
#undef AQ_GROUPED

std::atomic<unsigned long long*> g_aq_trace{nullptr};
std::atomic<int> g_aq_geometry{-1};  // tests / labs: -1 by shape, else a geometry id of the table above
std::atomic<int> g_aq_direct{-1};    // tests / labs: -1 the default, 0 the ring form of geometry 1 whatever the caller passes, else its direct form

inline int aq_direct_norm(int f) { return f == 0 ? 0 : AQ_DIRECT_STAGES; }
inline int aq_direct_stages() {
    static const int env = aq_direct_norm((int)env_int("SDNQ_HIP_FUSED_ROWQUANT_DIRECT", AQ_DIRECT_STAGES));  // tuning aid (0: the ring form)
    const int forced = g_aq_direct.load(std::memory_order_relaxed);
    return forced < 0 ? env : aq_direct_norm(forced);
}

constexpr int64_t AQ_TALL_MAX_K = 640;

// The launcher's choices for one problem, in one place (tests/test_gemm_aq_plan.py and test_gemm_aq_plan_tall.py hold the table this implements).
//   geometry 1 (32 x 256, 3 ring slots) where the front of the 64 x 128 tile -- ingest + quantization of 64 rows x K, repeated by every
//   column tile -- outweighs its K loop: int8, K of more than 5 stages, N a multiple of 256 (no column tile half empty), and one round:
//   at most one tile per CU.
//   the tall geometry (2: int8, K of at most 5 stages) where one round of 64 x 128 tiles, one per CU, does NOT cover the problem but
//   one round of the tall form does: at most `resident` tiles per CU.
//   Everything else keeps geometry 0 (64 x 128, 4 ring slots).
// A forced tall geometry on a problem it has no instantiation for (fp8, K > 640) falls back to the shape rule.
struct AqPlan { int geometry, bm, bn, tiles_m, tiles_n, group_m, resident; int64_t prefetch_room; };
inline AqPlan aq_plan(int mm_dtype, int64_t m, int64_t n, int64_t k, int cus) {
    static const int geo_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GEOMETRY", -1);  // tuning aid
    static const int gm_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GROUP_M", 8);     // tuning aid (1 = n fastest)
    static const int gm_tall_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GROUP_M_TALL", 8);  // the same for geometry 2
    struct Geo { int bm, bn, resident; };
    static constexpr Geo GEOS[3] = {{64, 128, 1}, {32, 256, 1}, {64, 128, 2}};
    const bool tall_ok = mm_dtype == SDNQ_MM_I8 && k <= AQ_TALL_MAX_K;
    auto tiles_of = [&](int g) { return ((m + GEOS[g].bm - 1) / GEOS[g].bm) * ((n + GEOS[g].bn - 1) / GEOS[g].bn); };
    int geo = g_aq_geometry.load(std::memory_order_relaxed);
    if (geo < 0) geo = geo_env;
    if (geo > 2 || (geo == 2 && !tall_ok)) geo = -1;
    if (geo < 0) {
        if (mm_dtype == SDNQ_MM_I8 && k > 640 && (n % 256) == 0 && ((m + 31) / 32) * (n / 256) <= cus) geo = 1;
        else if (tall_ok && tiles_of(0) > cus && tiles_of(2) <= (int64_t)GEOS[2].resident * cus) geo = 2;
        else geo = 0;
    }
    AqPlan pl;
    pl.geometry = geo;
    pl.bm = GEOS[geo].bm;
    pl.bn = GEOS[geo].bn;
    pl.resident = GEOS[geo].resident;
    pl.tiles_m = (int)((m + pl.bm - 1) / pl.bm);
    pl.tiles_n = (int)((n + pl.bn - 1) / pl.bn);
    // the walk groups 8 row blocks in every geometry.  32 x 256 at 1024 x 1280 x 1280: a group is 40 tiles = the 20 of two XCDs, each
    // 8 row blocks x 2.5 weight blocks; in the step 8 blocks ran 7.02 ms, 16 (the same ROWS as 8 of 64) 7.08, 2 / 4 / 6 7.04
    const int gm_e = geo == 2 ? gm_tall_env : gm_env;
    const int gm = gm_e < 1 ? 1 : gm_e;
    pl.group_m = gm > pl.tiles_m ? pl.tiles_m : gm;
    pl.prefetch_room = (int64_t)pl.resident * cus - (int64_t)pl.tiles_m * pl.tiles_n;  // workgroup slots (LDS) the tiles leave free
    return pl;
}

template <int X_T, int MM, bool HAS_BIAS, int NJ, int NSB, int BM, int BN, int RESIDENT = 1>
int launch_aq(const void* x, const void* w, int64_t ldx, int64_t m, int64_t n, int64_t k, const AqPlan& pl, AqParams p, hipStream_t s) {
    // the direct form (NSB < 0) has no ring, but asks for the three slots of the ring form all the same: one tile workgroup per CU, so
    // that the hosted prefetch workgroups (aq_plan's prefetch_room) never share a CU with a tile
    constexpr int LDS_BYTES = NJ * BM * BK + (NSB < 0 ? 3 : NSB) * BN * BK + (2 * BN + BM) * 4;
    static_assert(RESIDENT * LDS_BYTES <= 160 * 1024 && (RESIDENT + 1) * LDS_BYTES > 160 * 1024, "LDS budget: exactly RESIDENT workgroups per CU (aq_plan's prefetch room)");
    auto kern = linear_aq_kernel<X_T, MM, HAS_BIAS, NJ, NSB, BM, BN>;
    static std::atomic<uint64_t> attr_devices{0};
    if (LDS_BYTES > 64 * 1024 && !allow_dynamic_lds((const void*)kern, LDS_BYTES, attr_devices)) return SDNQ_ERR_LAUNCH;
    if (pl.bm != BM || pl.bn != BN || pl.resident != RESIDENT) return SDNQ_ERR_LAUNCH;
    const int tiles_m = pl.tiles_m, tiles_n = pl.tiles_n, group_m = pl.group_m;
    const int64_t tiles = (int64_t)tiles_m * tiles_n;
    p.trace = g_aq_trace.load(std::memory_order_relaxed);
    const int pf_wgs = sdnq_internal_take_prefetch(pl.prefetch_room, NT, p.pf_ptr, p.pf_lines);
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles + pf_wgs)), dim3(NT), LDS_BYTES, s, (const uint16_t*)x, (const uint8_t*)w, (int)ldx, (int)k, (int)m,
                       (int)n, (int)k, tiles_m, tiles_n, group_m, p);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

// ---- grouped launch: layers that read ONE activation (the linked q / k / v of a self-attention block) in one launch of the direct form ----
// Its tile is 32 x 256 with TWO workgroups per CU -- the direct form keeps no ring in LDS (40 KB image + vectors at K = 1280) and 117
// registers per lane, so a second tile is resident beside the first and its ingest, quantization and stores run under the first one's
// K loop; 1024 x (3 x 1280) is 480 tiles = one round on 240 CUs.  No flags or waits between workgroups: the hardware interleaves them.
// A 64 x 256 tile, one per CU (half the tiles and the weight traffic, twice the rows to quantize per wave, nothing resident beside it),
// was built and lost: -0.03 against -0.07 ... -0.11 ms in the step (profiles/linear_aq_qkv_grouped.txt).  Same bits
// as the row quantizer + grouped GEMM and as every member's own launch: tests/test_gemm_aq_grouped.py.
constexpr int AQ_GROUPED_BM = 32, AQ_GROUPED_BN = 256, AQ_GROUPED_RESIDENT = 2, AQ_GROUPED_NJ = 10;

// The rule of the grouped launch in one place (tests/test_gemm_aq_plan_grouped.py holds its table): int8 members of one width that is a
// multiple of the 256-column block, K of six to ten stages, and every tile of every member resident at once.  `ok` = 0: the group keeps
// the row-quantization launch and the grouped GEMM.
struct AqGroupPlan { int ok, bm, bn, tiles_m, tiles_n, group_m, resident; int64_t prefetch_room; };
inline AqGroupPlan aq_plan_grouped(int mm_dtype, int64_t m, int64_t n_member, int64_t n_members, int64_t k, int cus) {
    static const int gm_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GROUP_M", 8);             // the walk of aq_plan
    AqGroupPlan pl{};
    pl.bm = AQ_GROUPED_BM;
    pl.bn = AQ_GROUPED_BN;
    pl.resident = AQ_GROUPED_RESIDENT;
    if (mm_dtype != SDNQ_MM_I8 || m <= 0 || n_member <= 0 || (n_member % 256) != 0 || n_members < 1 || n_members > AQ_GROUP_MAX || (k % 128) != 0 ||
        k <= AQ_TALL_MAX_K || k > 1280 || cus <= 0)
        return pl;
    const int64_t tiles_m = (m + pl.bm - 1) / pl.bm, tiles_n = n_members * (n_member / 256);
    if (tiles_m * tiles_n > (int64_t)pl.resident * cus) return pl;
    pl.ok = 1;
    pl.tiles_m = (int)tiles_m;
    pl.tiles_n = (int)tiles_n;
    const int gm = gm_env < 1 ? 1 : gm_env;
    pl.group_m = gm > pl.tiles_m ? pl.tiles_m : gm;
    // hosted prefetch workgroups would share a CU with a tile here (two workgroups per CU): with the 2 * CUs - tiles slots handed out the
    // step ran 0.007 and 0.09 ms SLOWER than with none in two sessions (profiles/linear_aq_qkv_grouped.txt): no prefetch room
    pl.prefetch_room = 0;
    return pl;
}

template <int X_T, bool HAS_BIAS>
int launch_aq_grouped(const void* x, int64_t ldx, int64_t m, int64_t n_member, int64_t k, const AqGroupPlan& pl, AqParams p, const AqGroup& g, hipStream_t s) {
    constexpr int BM = AQ_GROUPED_BM, BN = AQ_GROUPED_BN, RESIDENT = AQ_GROUPED_RESIDENT, NJ = AQ_GROUPED_NJ;
    // what the tile uses -- the code image and the vectors; no ring --, raised to the smallest size of which RESIDENT + 1 do not fit a CU:
    // the count of co-resident workgroups is then RESIDENT whatever the register allocation (at 117 registers per lane two 8-wave
    // workgroups is also all the register file holds)
    constexpr int USED = NJ * BM * BK + (2 * BN + BM) * 4, FLOOR = (160 * 1024 / (RESIDENT + 1) / 1024 + 1) * 1024;
    constexpr int LDS_BYTES = USED > FLOOR ? USED : FLOOR;
    static_assert(RESIDENT * LDS_BYTES <= 160 * 1024 && (RESIDENT + 1) * LDS_BYTES > 160 * 1024, "LDS budget: exactly RESIDENT workgroups per CU");
    auto kern = linear_aq_grouped_kernel<X_T, SDNQ_MM_I8, HAS_BIAS, NJ, -AQ_DIRECT_STAGES, BM, BN>;
    static std::atomic<uint64_t> attr_devices{0};
    if (LDS_BYTES > 64 * 1024 && !allow_dynamic_lds((const void*)kern, LDS_BYTES, attr_devices)) return SDNQ_ERR_LAUNCH;
    if (!pl.ok) return SDNQ_ERR_LAUNCH;
    const int64_t tiles = (int64_t)pl.tiles_m * pl.tiles_n;
    p.trace = g_aq_trace.load(std::memory_order_relaxed);
    const int pf_wgs = sdnq_internal_take_prefetch(pl.prefetch_room, NT, p.pf_ptr, p.pf_lines);  // (no room: consumes a pending hint)
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles + pf_wgs)), dim3(NT), LDS_BYTES, s, (const uint16_t*)x, (int)ldx, (int)m, (int)n_member, (int)k, pl.tiles_m,
                       pl.tiles_n, pl.group_m, p, g);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

}  // namespace

// which problems take the one-launch route.  Costs that grow with it: tiles_n workgroups repeat the quantization of a row block (VALU
// time on the critical path of every tile), and a tile keeps its rows resident (K <= 1280).  Wins where the row-quantization launch
// is a large part of the pair: the one-round projections of the bs = 1 steps.  The rule: every tile of the problem resident at once --
// at most one 64 x 128 tile per CU, or, where those outnumber the CUs, a problem that aq_plan gives a tall geometry (int8, K <= 640,
// at most two co-resident tiles per CU: 4096 x 640 x 640 of the SDXL step).  A second round of tiles loses to the two launches.
extern "C" int sdnq_hip_linear_w8a8_fused_supported(int mm_dtype, int x_dtype, int out_dtype, int64_t m, int64_t n, int64_t k) {
    static const int64_t on = env_int("SDNQ_HIP_FUSED_ROWQUANT", 1), max_tn = env_int("SDNQ_HIP_FUSED_ROWQUANT_MAX_TILES_N", 12),
                         min_m = env_int("SDNQ_HIP_FUSED_ROWQUANT_MIN_M", 33), min_k = env_int("SDNQ_HIP_FUSED_ROWQUANT_MIN_K", 128),
                         max_k = env_int("SDNQ_HIP_FUSED_ROWQUANT_MAX_K", 1280);
    // fp8: built and bit-identical, off by default -- its quantization is costlier per element (sign fix-up, clamp, two converts per four
    // codes) and the SDXL fp8 step lost 2 % with it (7.08 -> 7.23 ms, profiles/r05_fused_rowquant_gemm.txt)
    static const int64_t fp8_on = env_int("SDNQ_HIP_FUSED_ROWQUANT_FP8", 0);
    if (!on) return 0;
    if (mm_dtype != SDNQ_MM_I8 && !(mm_dtype == SDNQ_MM_FP8 && fp8_on)) return 0;
    if ((x_dtype != SDNQ_BF16 && x_dtype != SDNQ_F16) || out_dtype != x_dtype) return 0;
    if (m < min_m || n <= 0 || (n % 8) != 0 || k <= 0 || (k % 128) != 0 || k > 1280) return 0;
    const int64_t tiles_m = (m + 63) / 64, tiles_n = (n + 127) / 128;  // (counted on the 64 x 128 tile, whichever geometry runs)
    if (tiles_n > max_tn || k < min_k || k > max_k) return 0;
    if (tiles_m * tiles_n > (int64_t)cu_count() && aq_plan(mm_dtype, m, n, k, cu_count()).geometry < 2) return 0;  // one round
    return 1;
}

namespace {
__global__ __launch_bounds__(256) void aq_slab_pack_kernel(const uint8_t* __restrict__ b, int64_t n, int nk, int64_t ldb, uint8_t* __restrict__ out, int64_t pieces) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one 16-byte piece per thread, in the order of the copy
    if (t >= pieces) return;
    const int l = (int)(t & 63), ks = (int)(t >> 6) & 3;
    const int64_t q = t >> 8, g = q / nk, j = q % nk;
    const int64_t row = g * 32 + (l & 31);
    const v4i v = *(const v4i*)(b + (row < n ? row : n - 1) * ldb + j * 128 + ks * 32 + (l >> 5) * 16);  // rows past N: the last row (never stored by a GEMM)
    *(v4i*)(out + t * 16) = v;
}
}  // namespace

extern "C" int64_t sdnq_hip_aq_slab_bytes(int64_t n, int64_t k) {
    if (n <= 0 || k <= 0 || (k % 128) != 0) return 0;
    return ((n + 31) / 32) * 32 * k;
}

extern "C" int sdnq_hip_aq_slab_wanted(int mm_dtype, int64_t m, int64_t n, int64_t k) {
    if (mm_dtype != SDNQ_MM_I8 || m <= 0 || n <= 0 || k <= 0 || (k % 128) != 0 || k > 1280) return 0;
    return aq_plan(mm_dtype, m, n, k, cu_count()).geometry == 1 && aq_direct_stages() != 0 ? 1 : 0;
}

extern "C" int sdnq_hip_aq_slab_pack(const void* b, int64_t n, int64_t k, int64_t ldb, void* out, sdnq_stream_t stream) {
    if (!b || !out) return SDNQ_ERR_NULL;
    if (n <= 0 || k <= 0 || ldb < k) return SDNQ_ERR_SHAPE;
    if ((k % 128) != 0 || k > 1280) return SDNQ_ERR_UNSUPPORTED;
    if (n > 0x7fffffffll / 2) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)b % 16) || ((uintptr_t)out % 16) || (ldb % 16)) return SDNQ_ERR_ALIGN;
    const int64_t pieces = sdnq_hip_aq_slab_bytes(n, k) / 16;
    hipLaunchKernelGGL(aq_slab_pack_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)b, n, (int)(k / 128), ldb,
                       (uint8_t*)out, pieces);
    SDNQ_CHECK_LAUNCH();
    return SDNQ_OK;
}

extern "C" int sdnq_hip_linear_w8a8_fused_slab(int mm_dtype, const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, const void* b,
                                               const float* sb, const void* bias, int bias_dtype, void* out, int out_dtype, int64_t n,
                                               const void* b_slab, sdnq_stream_t stream) {
    if (!x || !b || !sb || !out) return SDNQ_ERR_NULL;
    if (mm_dtype != SDNQ_MM_I8 && mm_dtype != SDNQ_MM_FP8) return SDNQ_ERR_DTYPE;
    if ((x_dtype != SDNQ_BF16 && x_dtype != SDNQ_F16) || out_dtype != x_dtype) return SDNQ_ERR_UNSUPPORTED;
    if (bias && (bias_dtype < 0 || bias_dtype > 2)) return SDNQ_ERR_DTYPE;
    if (m <= 0 || n <= 0 || k <= 0 || ldx < k || (n % 8) != 0) return SDNQ_ERR_SHAPE;
    if ((k % 128) != 0 || k > 1280) return SDNQ_ERR_UNSUPPORTED;
    if (m > 0x7fffffffll / 2 || n > 0x7fffffffll || ldx * 2 * 128 > 0x7fffffffll || k * 128 > 0x7fffffffll) return SDNQ_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((uintptr_t)b % 16) || ((uintptr_t)out % 16) || ((ldx * 2) % 16) || ((uintptr_t)b_slab % 16)) return SDNQ_ERR_ALIGN;
    AqParams p{};
    p.sb = sb; p.bias = bias; p.out = out; p.ldc = n; p.bias_dtype = bias_dtype;
    hipStream_t s = (hipStream_t)stream;
    const AqPlan pl = aq_plan(mm_dtype, m, n, k, cu_count());
    const bool direct = pl.geometry == 1 && mm_dtype == SDNQ_MM_I8 && b_slab != nullptr && aq_direct_stages() != 0;
    const void* const w = direct ? b_slab : b;
#define AQ_L(XT, MMV, HB, NJV, ...) launch_aq<XT, MMV, HB, NJV, __VA_ARGS__>(x, w, ldx, m, n, k, pl, p, s)
    // geometry 1 on int8 with the slab copy: the direct form, its register stages as the negative ring depth
#define AQ_D(XT, HB, NJV) AQ_L(XT, SDNQ_MM_I8, HB, NJV, -AQ_DIRECT_STAGES, 32, 256)
#define AQ_DB(XT, HB) (k <= 640 ? AQ_D(XT, HB, 5) : AQ_D(XT, HB, 10))
#define AQ_DX(XT) (bias ? AQ_DB(XT, true) : AQ_DB(XT, false))
    if (direct) return x_dtype == SDNQ_BF16 ? AQ_DX(SDNQ_BF16) : AQ_DX(SDNQ_F16);
#define AQ_G(XT, MMV, HB, NJV) (pl.geometry == 1 ? AQ_L(XT, MMV, HB, NJV, 3, 32, 256) : AQ_L(XT, MMV, HB, NJV, 4, 64, 128))
#define AQ_NJ(XT, MMV, HB) (k <= 640 ? AQ_G(XT, MMV, HB, 5) : AQ_G(XT, MMV, HB, 10))
#define AQ_B(XT, MMV) (bias ? AQ_NJ(XT, MMV, true) : AQ_NJ(XT, MMV, false))
#define AQ_X(MMV) (x_dtype == SDNQ_BF16 ? AQ_B(SDNQ_BF16, MMV) : AQ_B(SDNQ_F16, MMV))
    // the tall geometry: int8, five stages (aq_plan hands it out for nothing else)
#define AQ_TB(XT, ...) (bias ? AQ_L(XT, SDNQ_MM_I8, true, 5, __VA_ARGS__) : AQ_L(XT, SDNQ_MM_I8, false, 5, __VA_ARGS__))
#define AQ_T(...) (x_dtype == SDNQ_BF16 ? AQ_TB(SDNQ_BF16, __VA_ARGS__) : AQ_TB(SDNQ_F16, __VA_ARGS__))
    if (pl.geometry == 2) return AQ_T(2, 64, 128, 2);
    return mm_dtype == SDNQ_MM_I8 ? AQ_X(SDNQ_MM_I8) : AQ_X(SDNQ_MM_FP8);
#undef AQ_T
#undef AQ_TB
#undef AQ_X
#undef AQ_B
#undef AQ_NJ
#undef AQ_G
#undef AQ_DX
#undef AQ_DB
#undef AQ_D
#undef AQ_L
}

extern "C" int sdnq_hip_linear_w8a8_fused(int mm_dtype, const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, const void* b,
                                          const float* sb, const void* bias, int bias_dtype, void* out, int out_dtype, int64_t n,
                                          sdnq_stream_t stream) {
    return sdnq_hip_linear_w8a8_fused_slab(mm_dtype, x, x_dtype, m, k, ldx, b, sb, bias, bias_dtype, out, out_dtype, n, nullptr, stream);
}

// which groups take the grouped one-launch route: aq_plan_grouped's rule on this device, 16-bit activations in = out, and the switches of
// the single-layer route (SDNQ_HIP_FUSED_ROWQUANT, and SDNQ_HIP_FUSED_ROWQUANT_DIRECT: the grouped launch has the direct form only)
extern "C" int sdnq_hip_linear_w8a8_fused_grouped_supported(int mm_dtype, int x_dtype, int out_dtype, int64_t m, int64_t n_member, int64_t n_members,
                                                            int64_t k) {
    static const int64_t on = env_int("SDNQ_HIP_FUSED_ROWQUANT", 1) && env_int("SDNQ_HIP_FUSED_ROWQUANT_GROUPED", 1);
    if (!on || aq_direct_stages() == 0) return 0;
    if ((x_dtype != SDNQ_BF16 && x_dtype != SDNQ_F16) || out_dtype != x_dtype) return 0;
    return aq_plan_grouped(mm_dtype, m, n_member, n_members, k, cu_count()).ok;
}

extern "C" int sdnq_hip_linear_w8a8_fused_grouped(int mm_dtype, const void* x, int x_dtype, int64_t m, int64_t k, int64_t ldx, const void* const* b_slabs,
                                                  const float* const* sbs, const void* const* biases, int bias_dtype, int64_t n_members,
                                                  int64_t n_member, void* out, int out_dtype, sdnq_stream_t stream) {
    if (!x || !b_slabs || !sbs || !out) return SDNQ_ERR_NULL;
    if (mm_dtype != SDNQ_MM_I8) return SDNQ_ERR_UNSUPPORTED;
    if ((x_dtype != SDNQ_BF16 && x_dtype != SDNQ_F16) || out_dtype != x_dtype) return SDNQ_ERR_UNSUPPORTED;
    if (biases && (bias_dtype < 0 || bias_dtype > 2)) return SDNQ_ERR_DTYPE;
    if (m <= 0 || n_member <= 0 || n_members <= 0 || k <= 0 || ldx < k) return SDNQ_ERR_SHAPE;
    if (m > 0x7fffffffll / 2 || ldx * 2 * 128 > 0x7fffffffll) return SDNQ_ERR_SHAPE;
    const AqGroupPlan pl = aq_plan_grouped(mm_dtype, m, n_member, n_members, k, cu_count());
    if (!pl.ok) return SDNQ_ERR_UNSUPPORTED;
    if (((uintptr_t)x % 16) || ((uintptr_t)out % 16) || ((ldx * 2) % 16)) return SDNQ_ERR_ALIGN;
    AqGroup g{};
    g.bpm = (int)(n_member / 256);
    for (int64_t i = 0; i < n_members; ++i) {
        if (!b_slabs[i] || !sbs[i] || (biases && !biases[i])) return SDNQ_ERR_NULL;
        if ((uintptr_t)b_slabs[i] % 16) return SDNQ_ERR_ALIGN;
        g.slab[i] = (const uint8_t*)b_slabs[i];
        g.sb[i] = sbs[i];
        g.bias[i] = biases ? biases[i] : nullptr;
    }
    AqParams p{};
    p.out = out; p.ldc = n_member; p.bias_dtype = bias_dtype;
    hipStream_t s = (hipStream_t)stream;
#define AQ_GL(XT, HB) launch_aq_grouped<XT, HB>(x, ldx, m, n_member, k, pl, p, g, s)
#define AQ_GB(XT) (biases ? AQ_GL(XT, true) : AQ_GL(XT, false))
    return x_dtype == SDNQ_BF16 ? AQ_GB(SDNQ_BF16) : AQ_GB(SDNQ_F16);
#undef AQ_GB
#undef AQ_GL
}

// lab: phase stamps of the one-launch Linear (device buffer of 1024 x 8 uint64, or null to stop).  A C++ symbol internal to the library
// (tools/aq_lab.py binds its mangled name), not part of the C ABI of include/sdnq_hip.h
void sdnq_internal_aq_trace(unsigned long long* device_buf) { g_aq_trace.store(device_buf, std::memory_order_relaxed); }

// tests / labs: force the tile geometry of the one-launch Linear (-1 by shape, 0 = 64 x 128, 1 = 32 x 256, 2 = 64 x 128 on two ring
// slots; any other value = 1, as before the tall form); internal like the trace hook
void sdnq_internal_aq_geometry(int geometry) { g_aq_geometry.store(geometry < 0 ? -1 : (geometry <= 2 ? geometry : 1), std::memory_order_relaxed); }

// tests / labs: the form geometry 1 runs in on int8 where the caller passes the slab copy (-1 the default, 0 the LDS ring, any other value
// the direct form); internal like the hooks above
void sdnq_internal_aq_direct(int form) { g_aq_direct.store(form < 0 ? -1 : aq_direct_norm(form), std::memory_order_relaxed); }

// tests: what the launcher would choose for (mm_dtype, m, n, k) on a part with `cus` CUs:
// out = {geometry, BM, BN, tiles_m, tiles_n, group_m, prefetch room}
void sdnq_internal_aq_plan(int mm_dtype, long long m, long long n, long long k, int cus, long long* out) {
    const AqPlan pl = aq_plan(mm_dtype, m, n, k, cus);
    out[0] = pl.geometry; out[1] = pl.bm; out[2] = pl.bn; out[3] = pl.tiles_m; out[4] = pl.tiles_n; out[5] = pl.group_m; out[6] = pl.prefetch_room;
}

// tests: what the grouped launcher would choose for n_members members of n_member channels on a part with `cus` CUs:
// out = {accepted, BM, BN, tiles_m, tiles_n, group_m, resident, prefetch room}
void sdnq_internal_aq_plan_grouped(long long m, long long n_member, long long n_members, long long k, int cus, long long* out) {
    const AqGroupPlan pl = aq_plan_grouped(SDNQ_MM_I8, m, n_member, n_members, k, cus);
    out[0] = pl.ok; out[1] = pl.bm; out[2] = pl.bn; out[3] = pl.tiles_m; out[4] = pl.tiles_n; out[5] = pl.group_m; out[6] = pl.resident; out[7] = pl.prefetch_room;
}
