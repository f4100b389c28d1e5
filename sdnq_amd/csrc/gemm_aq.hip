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
// and two "tall" forms for K <= 640 (five stages held) where the 64 x 128 tiles of a problem outnumber the CUs:
//   2: 64 x 128, 2 ring slots : the tile of geometry 0 on a thin ring: 40 KB image + 32 KB ring, so TWO workgroups share a CU (the second
//                               one hides the first one's stage waits, as in the two-launch GEMM's 3 slots x 2 workgroups) and
//                               2 x CUs tiles are resident at once
//   3: 128 x 128, 3 ring slots: waves 2 x 4 with TWO 32 x 32 accumulators each (rows 64 wm .. + 64); a wave quantizes 16 rows in four
//                               passes; 80 KB image + 48 KB ring, one workgroup per CU, half the tiles
constexpr int BK = 128, NW = 8, NT = NW * 64;

struct AqParams {
    const float* sb;      // [N] weight row scales
    const void* bias;     // [N] or null
    void* out;            // [M][ldc]
    int64_t ldc;
    int bias_dtype;
    const uint8_t* pf_ptr[4];  // weight prefetch hosted by this launch (sdnq_hip_prefetch_hint)
    int pf_lines[4];
    unsigned long long* trace;  // lab: per-workgroup phase stamps (8 per workgroup), or null
#ifdef SDNQ_AQ_LAB
    int lab;  // lab build (timing only, results invalid): 1 no loop DMAs, 2 no fragment reads, 4 no MFMAs, 8 no barrier, 16 no quantization arithmetic
              // (the slab form of the 32 x 256 tile has no loop barrier and counts on every DMA: bits 1 and 8 do nothing there)
#endif
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

// X_T: activation dtype (bf16 / f16) = output dtype; NJ: K stages held (K <= 128 NJ); NSB: weight ring depth; BM x BN: tile geometry.
// NSB < 0 is the DIRECT form of the slab tile (int8): no LDS ring at all, -NSB weight stages in a ring of REGISTERS, loaded from the
// fragment-ordered copy of the weight (see DIRECT below)
template <int X_T, int MM, bool HAS_BIAS, int NJ, int NSB, int BM, int BN>
__global__ __launch_bounds__(NT) void linear_aq_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, int ldx, int ldb, int M, int N,
                                                       int K, int tiles_m, int tiles_n, int group_m, AqParams p_) {
    SDNQ_KERNARGS_NOW("s"(x), "s"(w), "s"(ldx), "s"(ldb), "s"(M), "s"(N), "s"(K), "s"(tiles_m), "s"(tiles_n), "s"(group_m));
    const AqParams& p = p_;
    typedef AqMma<MM> MT;
    constexpr int NACC = (BM / 32) * (BN / 32) / NW;  // 32x32 accumulators of a wave: consecutive row blocks of one column block
    static_assert(BM % 32 == 0 && BN % 32 == 0 && NACC * NW == (BM / 32) * (BN / 32) && NACC >= 1 && NACC <= 2, "one or two 32x32 accumulators per wave");
    constexpr int A_STAGE = BM * BK, B_STAGE = BN * BK;
    constexpr int PS = BM / (4 * NW);   // quantization passes of a wave: 4 rows (one per quarter wave) each
    constexpr int PPW = BN / (8 * NW);  // 1-KB ring pieces (8 weight rows) of a stage that one wave moves
    static_assert(PS >= 1 && PS <= 4 && PS * 4 * NW == BM && PPW >= 1 && PPW * 8 * NW == BN && BN <= NT, "geometry");
    // SLAB: every wave owns a private 32-column block (waves 1 x NW: geometry 1).  No weight byte is read by two waves, so a wave moves its
    // OWN 32 weight rows (pieces PPW w .. PPW w + PPW - 1 of every stage), takes each landed stage from its ring slot into registers,
    // refills the slot with stage j + NSB at once, and needs no barrier between the one that publishes the codes and the epilogue.
    constexpr bool SLAB = BN / 32 == NW;
    constexpr int KS = BK / MT::KB;
    static_assert(!SLAB || (NSB <= NJ && PPW == 4), "register slab: the ring is no deeper than the stages held; a wave's 32 rows are four pieces");
    // DIRECT: the slab form without the ring.  A wave's weight fragment of (stage j, sub-step ks) IS one 16-byte load per lane -- row
    // n0 + 32 wave + (lane & 31), bytes 128 j + 32 ks + 16 (lane >> 5) --, so the wave loads it from global memory straight into the
    // four registers the MFMA reads: no LDS-DMA piece to issue, no write into and fragment read out of LDS, no lgkmcnt wait before a
    // refill.  `w` is then the fragment-ordered COPY of the weight (sdnq_hip_aq_slab_pack: block g, stage j, sub-step ks at
    // ((g nk + j) 4 + ks) 1024, 16 bytes per lane), so that one load instruction reads 1 KiB = 8 lines; on the stored row-major operand
    // the same instruction touches 32 lines for 32 bytes each and the CU's address path takes 4 x as long over it (12.6 against 8.0 us
    // per launch, whatever the depth: DESIGN.md 7).  RD stages are in flight behind the activation rows; loads return in order, so the
    // counted vmcnt in front of a sub-step's MFMA (the compiler's: the fragments are ordinary values) lets stage 0 multiply while the
    // later stages are still on their way, and each fragment register is refilled with stage j + RD right behind the MFMA that read
    // it.  Stages and sub-steps in the ring form's order: the same bits (tests/test_gemm_aq_direct.py).
    constexpr bool DIRECT = NSB < 0;
    constexpr int RD = !DIRECT ? 0 : (-NSB < NJ ? -NSB : NJ);  // register stages: no more than the stages held
    constexpr int NSL = DIRECT ? 0 : NSB;                      // ring slots in LDS
    static_assert(!DIRECT || (SLAB && MM == SDNQ_MM_I8 && KS == 4 && RD >= 1 && KS * RD <= 48), "direct form: the int8 slab tile; the loads in flight fit the vmcnt counter");
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    uint8_t* const ldsA = lds;                       // [NJ][BM rows][128 B] quantized activation rows, resident
    uint8_t* const ldsB = lds + NJ * A_STAGE;        // [NSB][BN rows][128 B] weight ring
    float* const s_sb = (float*)(ldsB + NSL * B_STAGE);
    float* const s_bias = s_sb + BN;
    float* const s_xs = s_bias + BN;                 // [BM] activation row scales

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwg = tiles_m * tiles_n;
    const int bid = blockIdx.x;
    if (bid >= nwg) {  // hosted weight prefetch
        SDNQ_PREFETCH_LINES(tid, bid - nwg, NT, (int)gridDim.x - nwg, p);
        return;
    }
    const unsigned long long t_entry = __builtin_amdgcn_s_memtime();  // (stored with stamp 1: nothing waits for the trace pointer before the loads go out)
    int tile_m, tile_n;
    grouped_tile(xcd_contiguous(bid, nwg), tiles_m, tiles_n, group_m, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk = K / BK;  // (launcher: K % 128 == 0, K <= 128 NJ)
    const int m_rows = (M - m0) < BM ? (M - m0) : BM, n_lim = (N - n0) < BN ? (N - n0) : BN;

    // ---- activation rows: every load of the wave's 8 rows in flight before anything else ---------------------------------------------
    const auto rsX = SDNQ_MAKE_RSRC_N((const uint8_t*)x + (int64_t)m0 * ldx * 2, ((int64_t)(m_rows - 1) * ldx + K) * 2);
    v4i xr[PS][NJ];
    int qrow[PS];
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        qrow[ps] = wave * (4 * PS) + ps * 4 + (lane >> 4);
        const int rc = qrow[ps] < m_rows ? qrow[ps] : m_rows - 1;  // rows past M: computed on valid memory, never stored
        const int vo = rc * ldx * 2 + (lane & 15) * 16;
#pragma unroll
        for (int j = 0; j < NJ; ++j) xr[ps][j] = SDNQ_BUF_LOAD16(rsX, vo, j < nk ? j * 256 : 0x40000000);  // stages past K: out of range = zeros
    }
    // ---- weight ring prologue: piece = 8 rows x 128 B, lane l -> row l / 8, physical chunk l % 8 (source chunk = swizzle-inverse);
    // wave w owns pieces w, w + 8, ... (PPW of them) of every stage -- in the register-slab form pieces PPW w ..: its own 32 weight rows;
    // constant per-lane offsets, the K advance in the scalar operand
    // (direct form: the descriptor spans the 32-row blocks of this tile that exist in the copy)
    const int nblk = (n_lim + 31) >> 5;
    const auto rsB = DIRECT ? SDNQ_MAKE_RSRC_N(w + (int64_t)tile_n * (BN / 32) * nk * 4096, nblk * nk * 4096)
                            : SDNQ_MAKE_RSRC_N(w + (int64_t)n0 * ldb, (int64_t)(n_lim - 1) * ldb + K);
    int voB[PPW];
    auto pieceB = [&](int u) { return SLAB ? wave * PPW + u : wave + u * NW; };
#pragma unroll
    for (int u = 0; u < PPW; ++u) {
        const int r = pieceB(u) * 8 + (lane >> 3);
        const int rc = r < n_lim ? r : n_lim - 1;
        voB[u] = rc * ldb + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    }
    auto issueB = [&](int st, int slot) {  // stages past the end re-fetch stage 0 (never consumed; keeps the counted vmcnt a constant)
        const int s = st < nk ? st : 0;
#pragma unroll
        for (int u = 0; u < PPW; ++u) SDNQ_DMA16(rsB, ldsB + slot * B_STAGE + pieceB(u) * 1024, voB[u], s * BK);
    };
    constexpr int AHEAD = DIRECT ? RD : (SLAB ? NSB : NSB - 1);  // stages in flight behind the rows (the slab forms have no slot to hold back: they refill as they drain)
    // direct form: the wave's own block of the copy, one fragment per load; a wave whose block lies past N reads the tile's last block
    // (valid memory, never stored)
    typename MT::frag_t fbd[DIRECT ? RD : 1][KS];
    const int voD = lane << 4, soD = (wave < nblk ? wave : nblk - 1) * nk * 4096;
    auto issueD = [&](auto slotc, auto ksc, int st) {  // stages past the end re-fetch stage 0, as issueB does (never multiplied)
        constexpr int ks = decltype(ksc)::value;
        if constexpr (DIRECT) fbd[decltype(slotc)::value][ks] = SDNQ_BUF_LOAD16(rsB, voD, soD + (st < nk ? st : 0) * 4096 + ks * 1024);
    };
    if constexpr (DIRECT) {
        // (pinned one by one: the counted waits of the K loop follow the order of issue, and the scheduler put stage 1 in front of stage 0's last sub-step)
        static_for_up<RD>([&](auto sc) {
            static_for_up<KS>([&](auto ksc) {
                issueD(sc, ksc, decltype(sc)::value);
                __builtin_amdgcn_sched_barrier(0);
            });
        });
    } else {
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) issueB(s, s);
    }
    __builtin_amdgcn_sched_barrier(0);
    SDNQ_KERNARGS_NOW("s"(p_.sb), "s"(p_.bias), "s"(p_.out), "s"(p_.ldc), "s"(p_.bias_dtype), "s"(p_.trace));
    if (p.trace != nullptr && tid == 0 && blockIdx.x < 1024) p.trace[blockIdx.x * 8] = t_entry;
    SDNQ_PHASE_STAMP(p.trace, 1);
    // per-channel epilogue vectors: requested now (behind the rows and the ring prologue), parked in LDS after the quantization
    float ev_sb = 0.0f;
    u32 ev_bias = 0;  // raw bits: converted when parked (a conversion here would wait for every load in flight)
    if (tid < BN) {
        const int64_t gi = n0 + (tid < n_lim ? tid : n_lim - 1);
        ev_sb = p.sb[gi];
        if constexpr (HAS_BIAS) {
            if (p.bias_dtype == SDNQ_F32) ev_bias = ((const u32*)p.bias)[gi];
            else ev_bias = ((const uint16_t*)p.bias)[gi];
        }
    }

    // ---- row quantization: amax inside the 16-lane row group, IEEE scale, lean codes -> the resident LDS image -------------------------
    constexpr float QMAX = (MM == SDNQ_MM_I8) ? 127.0f : 448.0f;
    // slab form, draining weight stage j: the wave waits for its own four pieces of the stage -- loads return in order, so a count of the
    // pieces issued after them --, reads its KS fragments out of the ring slot into `dst` and, those reads retired, refills the slot with
    // stage j + NSB.  Stages past K are issued all the same (issueB's filler: the counts stay constants) and never read.
    // The first DF stages are drained under the quantization, behind the codes of its last DF stages, into registers of their own (16 per
    // stage, statically indexed); every later stage in the K loop, in front of its MFMAs.  DF = 2 measured best in the step: 0 leaves the
    // fill path idle behind the three prologue stages, 3 / 4 / all ten hold up the quantization -- and with it the barrier every wave's
    // MFMAs wait for -- on weights that have not landed yet (profiles/linear_aq_32x256_regslab.txt).
    constexpr int DF = !SLAB || DIRECT ? 0 : (NJ < 2 ? NJ : 2);
    typename MT::frag_t fbr[DF > 0 ? DF : 1][KS], fbs[KS];
    auto drainB = [&](int j, typename MT::frag_t* dst) {
        if (j < nk) {
            static_for_up<NJ>([&](auto jc) {
                constexpr int later = NJ - 1 - decltype(jc)::value;  // stages issued behind stage j so far
                if (decltype(jc)::value == j) wait_vmcnt<PPW * (later < NSB - 1 ? later : NSB - 1)>();
            });
#ifdef SDNQ_AQ_LAB
            if (!(p.lab & 2))
#endif
            static_for_up<KS>([&](auto ksc) { dst[decltype(ksc)::value] = MT::load(ldsB + (j % NSB) * B_STAGE, wave * 32 + (lane & 31), decltype(ksc)::value, lane >> 5); });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (j + NSB < NJ) issueB(j + NSB, j % NSB);
    };
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        // loads return in order: a pass has landed when at most the NJ loads of each later pass and this wave's PPW AHEAD ring pieces are outstanding
        static_for_up<PS>([&](auto pc) {
            if (decltype(pc)::value == ps) wait_vmcnt<(PS - 1 - decltype(pc)::value) * NJ + PPW * AHEAD>();
        });
        // |x| of 16-bit floats orders like the unsigned integer of its low 15 bits: packed integer max, two elements per instruction
        us2 mx = {0, 0};
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int d = 0; d < 4; ++d)
                mx = __builtin_elementwise_max(mx, __builtin_bit_cast(us2, (u32)xr[ps][j][d] & 0x7fff7fffu));
        u32 m32 = __builtin_bit_cast(u32, mx);
#pragma unroll
        for (int s = 1; s <= 8; s <<= 1) {
            const u32 o = (u32)lane_xor_i32((int)m32, s);
            m32 = __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(us2, m32), __builtin_bit_cast(us2, o)));
        }
        u32 mb = (m32 & 0xffffu) > (m32 >> 16) ? (m32 & 0xffffu) : (m32 >> 16);
        // a NaN orders above everything here, but the row quantizer's fmaxf drops it (rowquant.hip): a row that holds one takes its amax
        // over the other elements, as there.  Off the ordinary path: one compare per pass, the second sweep only for such a row's wave.
        constexpr u32 INF_BITS = X_T == SDNQ_BF16 ? 0x7f80u : 0x7c00u;
        if (__builtin_amdgcn_ballot_w64(mb > INF_BITS) != 0) {
            u32 mn = 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const u32 lo = (u32)xr[ps][j][d] & 0x7fffu, hi = ((u32)xr[ps][j][d] >> 16) & 0x7fffu;
                    mn = lo > INF_BITS ? mn : (lo > mn ? lo : mn);
                    mn = hi > INF_BITS ? mn : (hi > mn ? hi : mn);
                }
#pragma unroll
            for (int s = 1; s <= 8; s <<= 1) {
                const u32 o = (u32)lane_xor_i32((int)mn, s);
                mn = o > mn ? o : mn;
            }
            mb = mn;
        }
        const float amax = X_T == SDNQ_BF16 ? __uint_as_float(mb << 16) : f16_bits_to_f32((uint16_t)mb);
        const float scale = amax / QMAX;  // get_scale_symmetric, quant_utils.py:23-24
        RowDiv rd;
        rd.set(scale);
        if ((lane & 15) == 0) s_xs[qrow[ps]] = scale;
        const int r = qrow[ps];
        uint8_t* dst = ldsA + r * 128 + ((lane & 1) << 3) + ((((lane & 15) >> 1) ^ ((r >> 1) & 7)) << 4);
        // one test per pass, not per chunk: every row of the wave on the lean path (scale finite and ordinary -- anything but an all-zero
        // / inf / nan row), else the general path for all four rows (same codes: quant8 takes the same lean branch lane by lane)
        const bool all_fast = __builtin_amdgcn_ballot_w64(!rd.fast) == 0;
#ifdef SDNQ_AQ_LAB
        if (p.lab & 16) {
            if constexpr (SLAB) {
                if (ps == PS - 1) {
#pragma unroll
                    for (int j = 0; j < DF; ++j) drainB(j, fbr[j]);
                }
            }
            continue;
        }
#endif
        if (all_fast) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float v[8];
                const v4i t = xr[ps][j];
                Vec16<X_T>::unpack(make_uint4((u32)t[0], (u32)t[1], (u32)t[2], (u32)t[3]), v);
                const uint2 q = quant8_fast<MM>(v, rd);
                *(v2i*)(dst + j * A_STAGE) = (v2i){(int)q.x, (int)q.y};  // (ext-vector store: a HIP-struct store drains the LDS-DMAs first)
                if constexpr (DF > 0) { if (ps == PS - 1 && j >= NJ - DF) drainB(j - (NJ - DF), fbr[j - (NJ - DF)]); }
            }
        } else {  // (unrolled as well: a run-time index into the row registers would put them in scratch memory)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float v[8];
                const v4i t = xr[ps][j];
                Vec16<X_T>::unpack(make_uint4((u32)t[0], (u32)t[1], (u32)t[2], (u32)t[3]), v);
                int isum = 0;
                const uint2 q = quant8<MM>(v, rd, isum);
                *(v2i*)(dst + j * A_STAGE) = (v2i){(int)q.x, (int)q.y};
                if constexpr (DF > 0) { if (ps == PS - 1 && j >= NJ - DF) drainB(j - (NJ - DF), fbr[j - (NJ - DF)]); }
            }
        }
    }
    // the per-channel vectors are parked here -- in the slab form behind the K loop: they were requested behind the ring prologue, and a
    // wait for them in front of the loop would wait for every prologue stage of the wave as well
    if (tid < BN && !SLAB) {
        s_sb[tid] = ev_sb;
        if constexpr (HAS_BIAS)
            s_bias[tid] = p.bias_dtype == SDNQ_F32 ? __uint_as_float(ev_bias) : (p.bias_dtype == SDNQ_BF16 ? __uint_as_float(ev_bias << 16) : f16_bits_to_f32((uint16_t)ev_bias));
    }
    SDNQ_PHASE_STAMP(p.trace, 2);

    // ---- K loop: weight stages through the ring, activation fragments from the resident image ----------------------------------------
    typename MT::acc_t acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a][e] = 0;
    const int wm = (wave / (BN / 32)) * NACC, wn = wave % (BN / 32);  // first 32-row block, 32-column block of the wave
    const int frow = lane & 31, fgrp = lane >> 5;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's codes and scales are in LDS before the first barrier lets anyone read them
#ifdef SDNQ_AQ_LAB
    const int lab = __builtin_amdgcn_readfirstlane(p.lab);
#else
    constexpr int lab = 0;  // (run-time switches inside the K loop cost it 35 %: a lab build only)
#endif
    typename MT::frag_t fa[2][NACC][KS];
    if constexpr (DIRECT) {
        // Direct form: the slab loop below with the weight fragments already in registers.  Sub-step ks of stage kt multiplies
        // fbd[kt % RD][ks] as soon as that load has landed, and the register is reloaded with the same sub-step of stage kt + RD.
        auto read_a = [&](auto setc, auto ksc, int st) {
            constexpr int sx = decltype(setc)::value, ks = decltype(ksc)::value;
#pragma unroll
            for (int a = 0; a < NACC; ++a) fa[sx][a][ks] = MT::load(ldsA + (st < nk ? st : 0) * A_STAGE, (wm + a) * 32 + frow, ks, fgrp);
        };
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        static_for_up<KS>([&](auto ksc) { read_a(std::integral_constant<int, 0>{}, ksc, 0); });
        static_for_up<NJ>([&](auto ktc) {
            constexpr int kt = decltype(ktc)::value, sx = kt & 1, slot = kt % (RD > 0 ? RD : 1);
            if (kt < nk) {
                __builtin_amdgcn_sched_barrier(0);
                static_for_up<KS>([&](auto ksc) {
                    constexpr int ks = decltype(ksc)::value;
                    if (!(lab & 4)) {
#pragma unroll
                        for (int a = 0; a < NACC; ++a) MT::mma(acc[a], fbd[slot][ks], fa[sx][a][ks]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (kt + 1 < NJ) { if (!(lab & 2)) read_a(std::integral_constant<int, sx ^ 1>{}, ksc, kt + 1); }
                    if constexpr (kt + RD < NJ) issueD(std::integral_constant<int, slot>{}, ksc, kt + RD);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    } else if constexpr (SLAB) {
        // Slab form: the one barrier below publishes the A image; behind it a wave depends on nobody -- it waits for its OWN pieces of a
        // stage (counted vmcnt), takes them into registers, refills the slot and multiplies, so the waves drift apart and every wave
        // keeps NSB stages in flight of its own accord (the ring form refills a slot only once all eight waves have left it).  Stages
        // 0 .. nk - 1 and their sub-steps in the ring form's order: the accumulation order of every element is the same.  The A
        // fragments stay software-pipelined one stage deep over two register sets (the stage count is a template constant: unrolled).
        auto read_a = [&](auto setc, auto ksc, int st) {
            constexpr int sx = decltype(setc)::value, ks = decltype(ksc)::value;
#pragma unroll
            for (int a = 0; a < NACC; ++a) fa[sx][a][ks] = MT::load(ldsA + (st < nk ? st : 0) * A_STAGE, (wm + a) * 32 + frow, ks, fgrp);
        };
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        static_for_up<KS>([&](auto ksc) { read_a(std::integral_constant<int, 0>{}, ksc, 0); });
        static_for_up<NJ>([&](auto ktc) {
            constexpr int kt = decltype(ktc)::value, sx = kt & 1;
            if (kt < nk) {
                if constexpr (kt >= DF) drainB(kt, fbs);
                __builtin_amdgcn_sched_barrier(0);
                static_for_up<KS>([&](auto ksc) {
                    constexpr int ks = decltype(ksc)::value;
                    if (!(lab & 4)) {
#pragma unroll
                        for (int a = 0; a < NACC; ++a) MT::mma(acc[a], kt < DF ? fbr[kt < DF ? kt : 0][ks] : fbs[ks], fa[sx][a][ks]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (kt + 1 < NJ) { if (!(lab & 2)) read_a(std::integral_constant<int, sx ^ 1>{}, ksc, kt + 1); }
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    } else {
        // Software pipeline one STAGE deep (the LD_OV form of gemm.hip, profiles/r05_overlapped_ring_lab.txt): the fragments of stage kt sit in
        // registers when its barrier falls, so the MFMAs start at once; dealt out between them are the fragment reads of stage kt + 1 (which that
        // barrier published) and the DMA pieces of stage kt + NSB into the slot stage kt has just vacated -- NSB - 1 stages in flight behind the
        // landed one.  Two register sets, so the loop is unrolled by two.
        typename MT::frag_t fb[2][KS];
        auto read_stage = [&](auto setc, auto ksc, int st, int slot) {
            constexpr int sx = decltype(setc)::value, ks = decltype(ksc)::value;
#pragma unroll
            for (int a = 0; a < NACC; ++a) fa[sx][a][ks] = MT::load(ldsA + (st < nk ? st : 0) * A_STAGE, (wm + a) * 32 + frow, ks, fgrp);
            fb[sx][ks] = MT::load(ldsB + slot * B_STAGE, wn * 32 + frow, ks, fgrp);
        };
        wait_vmcnt<(AHEAD - 1) * PPW>();  // stage 0 (this wave's pieces; the barrier makes it everybody's)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        issueB(AHEAD, AHEAD);              // the ring's last free slot
        static_for_up<KS>([&](auto ksc) { read_stage(std::integral_constant<int, 0>{}, ksc, 0, 0); });
        int slot_c = 0;  // ring slot of the stage whose fragments are in registers
        auto half = [&](auto setc, int kt) {
            constexpr int sx = decltype(setc)::value;
            wait_vmcnt<(NSB - 2) * PPW>();                     // this wave's pieces of stage kt + 1 have landed
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and its reads of stage kt have retired: the slot may be refilled
            __builtin_amdgcn_sched_barrier(0);
            if (!(lab & 8)) __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            const int slot_free = slot_c;
            slot_c = (slot_c + 1 == NSB) ? 0 : slot_c + 1;
            // MFMA ks of stage kt, then read ks of stage kt + 1 (the last sub-step's reads retire under the next barrier's wait; KS <= 4)
            static_for_up<KS>([&](auto ksc) {
                constexpr int ks = decltype(ksc)::value;
                if (!(lab & 4)) {
#pragma unroll
                    for (int a = 0; a < NACC; ++a) MT::mma(acc[a], fb[sx][ks], fa[sx][a][ks]);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (!(lab & 2)) read_stage(std::integral_constant<int, sx ^ 1>{}, ksc, kt + 1, slot_c);
                if constexpr (ks == 0) { if (!(lab & 1)) issueB(kt + NSB, slot_free); }
                __builtin_amdgcn_sched_barrier(0);
            });
        };
#pragma nounroll
        for (int kt = 0; kt < nk; kt += 2) {
            half(std::integral_constant<int, 0>{}, kt);
            if (kt + 1 < nk) half(std::integral_constant<int, 1>{}, kt + 1);
        }
    }
    SDNQ_PHASE_STAMP(p.trace, 3);
    if (tid < BN && SLAB) {  // (the barrier below publishes them to the epilogue)
        s_sb[tid] = ev_sb;
        if constexpr (HAS_BIAS)
            s_bias[tid] = p.bias_dtype == SDNQ_F32 ? __uint_as_float(ev_bias) : (p.bias_dtype == SDNQ_BF16 ? __uint_as_float(ev_bias << 16) : f16_bits_to_f32((uint16_t)ev_bias));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing filler DMAs target the ring; the staging area below is the A image
    __syncthreads();                                  // every wave is done with the A image before it becomes the output staging area
    SDNQ_PHASE_STAMP(p.trace, 4);

    // ---- epilogue in the MFMA register layout: lane owns row wm*32 + (lane & 31), channels wn*32 + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5);
    // out = cast(fma(f32(acc) * xs, ws, bias)) (kernel_wrappers.py:132-144); final 16-bit values leave through LDS as 16-byte row pieces
    constexpr int OUT_ROW = BN * 2 + 16;
    static_assert(BM * OUT_ROW <= NJ * A_STAGE + NSL * B_STAGE, "output staging fits the operand area");
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const int ml = (wm + a) * 32 + frow;
        const float sa = s_xs[ml];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nl0 = wn * 32 + 8 * q + 4 * fgrp;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float vv = MT::tof(acc[a], 4 * q + e) * sa;
                if constexpr (HAS_BIAS) o[e] = fmaf(vv, s_sb[nl0 + e], s_bias[nl0 + e]);
                else o[e] = vv * s_sb[nl0 + e];
            }
            *(uint2*)(lds + ml * OUT_ROW + nl0 * 2) = make_uint2(pack2<X_T>(o[0], o[1]), pack2<X_T>(o[2], o[3]));
        }
    }
    __syncthreads();
    SDNQ_PHASE_STAMP(p.trace, 5);
    constexpr int PPR = BN * 2 / 16;  // 16-byte pieces per output row
#pragma unroll
    for (int v = tid; v < BM * PPR; v += NT) {
        const int r = v / PPR, c = v % PPR;
        if (r >= m_rows || c * 8 >= n_lim) continue;  // N % 8 == 0: a piece never straddles N
        const uint4 val = *(const uint4*)(lds + r * OUT_ROW + c * 16);
        __builtin_nontemporal_store((v4i){(int)val.x, (int)val.y, (int)val.z, (int)val.w},
                                    (v4i*)((uint8_t*)p.out + ((int64_t)(m0 + r) * p.ldc + n0 + c * 8) * 2));
    }
    SDNQ_PHASE_STAMP(p.trace, 6);
}

std::atomic<unsigned long long*> g_aq_trace{nullptr};
std::atomic<int> g_aq_geometry{-1};  // tests / labs: -1 by shape, else a geometry id of the table above
std::atomic<int> g_aq_direct{-1};    // tests / labs: -1 the default, 0 the ring form of geometry 1 whatever the caller passes, else its direct form

// The form geometry 1 runs in on int8 where the caller passes the slab copy of the weight (sdnq_hip_linear_w8a8_fused_slab): the direct
// form with AQ_DIRECT_STAGES register stages, or 0: the LDS ring (as without a copy).  Depths 3, 4, 6 and 8 were built and measured in
// the step: 3 and 4 level, 6 and 8 behind; 3 takes the fewest registers.
constexpr int AQ_DIRECT_STAGES = 3;
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
//   a tall geometry (2 or 3: int8, K of at most 5 stages) where one round of 64 x 128 tiles, one per CU, does NOT cover the problem but
//   one round of the tall form does: at most `resident` tiles per CU.
//   Everything else keeps geometry 0 (64 x 128, 4 ring slots).
// A forced tall geometry on a problem it has no instantiation for (fp8, K > 640) falls back to the shape rule.
struct AqPlan { int geometry, bm, bn, tiles_m, tiles_n, group_m, resident; int64_t prefetch_room; };
inline AqPlan aq_plan(int mm_dtype, int64_t m, int64_t n, int64_t k, int cus) {
    static const int geo_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GEOMETRY", -1);  // tuning aid
    static const int gm_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GROUP_M", 8);     // tuning aid (1 = n fastest)
    static const int gm_tall_env = (int)env_int("SDNQ_HIP_FUSED_ROWQUANT_GROUP_M_TALL", 8);  // the same for geometries 2 and 3
    // the tall form the shape rule picks: 2 (3 lost in the step; the variable is how that was measured)
    static const int tall = env_int("SDNQ_HIP_FUSED_ROWQUANT_TALL_GEOMETRY", 2) == 3 ? 3 : 2;
    struct Geo { int bm, bn, resident; };
    static constexpr Geo GEOS[4] = {{64, 128, 1}, {32, 256, 1}, {64, 128, 2}, {128, 128, 1}};
    const bool tall_ok = mm_dtype == SDNQ_MM_I8 && k <= AQ_TALL_MAX_K;
    auto tiles_of = [&](int g) { return ((m + GEOS[g].bm - 1) / GEOS[g].bm) * ((n + GEOS[g].bn - 1) / GEOS[g].bn); };
    int geo = g_aq_geometry.load(std::memory_order_relaxed);
    if (geo < 0) geo = geo_env;
    if (geo > 3 || (geo >= 2 && !tall_ok)) geo = -1;
    if (geo < 0) {
        if (mm_dtype == SDNQ_MM_I8 && k > 640 && (n % 256) == 0 && ((m + 31) / 32) * (n / 256) <= cus) geo = 1;
        else if (tall_ok && tiles_of(0) > cus && tiles_of(tall) <= (int64_t)GEOS[tall].resident * cus) geo = tall;
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
    const int gm_e = geo >= 2 ? gm_tall_env : gm_env;
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
#ifdef SDNQ_AQ_LAB
    p.lab = (int)env_int("SDNQ_HIP_AQ_LAB", 0);
#endif
    const int pf_wgs = sdnq_internal_take_prefetch(pl.prefetch_room, NT, p.pf_ptr, p.pf_lines);
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles + pf_wgs)), dim3(NT), LDS_BYTES, s, (const uint16_t*)x, (const uint8_t*)w, (int)ldx, (int)k, (int)m,
                       (int)n, (int)k, tiles_m, tiles_n, group_m, p);
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
    // the tall geometries: int8, five stages (aq_plan hands them out for nothing else)
#define AQ_TB(XT, ...) (bias ? AQ_L(XT, SDNQ_MM_I8, true, 5, __VA_ARGS__) : AQ_L(XT, SDNQ_MM_I8, false, 5, __VA_ARGS__))
#define AQ_T(...) (x_dtype == SDNQ_BF16 ? AQ_TB(SDNQ_BF16, __VA_ARGS__) : AQ_TB(SDNQ_F16, __VA_ARGS__))
    if (pl.geometry == 2) return AQ_T(2, 64, 128, 2);
    if (pl.geometry == 3) return AQ_T(3, 128, 128, 1);
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

// lab: phase stamps of the one-launch Linear (device buffer of 1024 x 8 uint64, or null to stop).  A C++ symbol internal to the library
// (tools/aq_lab.py binds its mangled name), not part of the C ABI of include/sdnq_hip.h
void sdnq_internal_aq_trace(unsigned long long* device_buf) { g_aq_trace.store(device_buf, std::memory_order_relaxed); }

// tests / labs: force the tile geometry of the one-launch Linear (-1 by shape, 0 = 64 x 128, 1 = 32 x 256, 2 = 64 x 128 on two ring
// slots, 3 = 128 x 128; any other value = 1, as before the tall forms); internal like the trace hook
void sdnq_internal_aq_geometry(int geometry) { g_aq_geometry.store(geometry < 0 ? -1 : (geometry <= 3 ? geometry : 1), std::memory_order_relaxed); }

// tests / labs: the form geometry 1 runs in on int8 where the caller passes the slab copy (-1 the default, 0 the LDS ring, any other value
// the direct form); internal like the hooks above
void sdnq_internal_aq_direct(int form) { g_aq_direct.store(form < 0 ? -1 : aq_direct_norm(form), std::memory_order_relaxed); }

// tests: what the launcher would choose for (mm_dtype, m, n, k) on a part with `cus` CUs:
// out = {geometry, BM, BN, tiles_m, tiles_n, group_m, prefetch room}
void sdnq_internal_aq_plan(int mm_dtype, long long m, long long n, long long k, int cus, long long* out) {
    const AqPlan pl = aq_plan(mm_dtype, m, n, k, cus);
    out[0] = pl.geometry; out[1] = pl.bm; out[2] = pl.bn; out[3] = pl.tiles_m; out[4] = pl.tiles_n; out[5] = pl.group_m; out[6] = pl.prefetch_room;
}
