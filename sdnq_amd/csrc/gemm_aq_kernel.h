// linear_aq_kernel of gemm_aq.hip (its header comment is there) and its grouped form.
// No include guard: the unit includes this file once per form, with AQ_GROUPED 0 (the single-layer kernel, whose text -- and therefore
// whose code -- is what it was before the grouped form existed) and with AQ_GROUPED 1 (linear_aq_grouped_kernel: the direct form for
// several layers that read one activation; only the base pointers of a tile differ -- the lines between #if AQ_GROUPED).
//
// X_T: activation dtype (bf16 / f16) = output dtype; NJ: K stages held (K <= 128 NJ); NSB: weight ring depth; BM x BN: tile geometry.
// NSB < 0 is the DIRECT form of the slab tile (int8): no LDS ring at all, -NSB weight stages in a ring of REGISTERS, loaded from the
// fragment-ordered copy of the weight (see DIRECT below)
#if AQ_GROUPED
// grouped: N is ONE member's width, tiles_n counts the column blocks of every member, g_ names the members (AqGroup in gemm_aq.hip)
template <int X_T, int MM, bool HAS_BIAS, int NJ, int NSB, int BM, int BN>
__global__ __launch_bounds__(NT) void linear_aq_grouped_kernel(const uint16_t* __restrict__ x, int ldx, int M, int N, int K, int tiles_m, int tiles_n,
                                                               int group_m, AqParams p_, AqGroup g_) {
    SDNQ_KERNARGS_NOW("s"(x), "s"(ldx), "s"(M), "s"(N), "s"(K), "s"(tiles_m), "s"(tiles_n), "s"(group_m), "s"(g_.bpm));
    static_assert(NSB < 0, "a grouped launch runs the direct form");
    constexpr int ldb = 0;  // (the stored operand's row stride: the ring forms only)
#else
template <int X_T, int MM, bool HAS_BIAS, int NJ, int NSB, int BM, int BN>
__global__ __launch_bounds__(NT) void linear_aq_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, int ldx, int ldb, int M, int N,
                                                       int K, int tiles_m, int tiles_n, int group_m, AqParams p_) {
    SDNQ_KERNARGS_NOW("s"(x), "s"(w), "s"(ldx), "s"(ldb), "s"(M), "s"(N), "s"(K), "s"(tiles_m), "s"(tiles_n), "s"(group_m));
#endif
    const AqParams& p = p_;
    typedef AqMma<MM> MT;
    static_assert(BM % 32 == 0 && BN % 32 == 0 && (BM / 32) * (BN / 32) == NW, "one 32x32 accumulator per wave");
    constexpr int A_STAGE = BM * BK, B_STAGE = BN * BK;
    constexpr int PS = BM / (4 * NW);   // quantization passes of a wave: 4 rows (one per quarter wave) each
    constexpr int PPW = BN / (8 * NW);  // 1-KB ring pieces (8 weight rows) of a stage that one wave moves
    static_assert(PS >= 1 && PS <= 2 && PS * 4 * NW == BM && PPW >= 1 && PPW * 8 * NW == BN && BN <= NT, "geometry");
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
#if AQ_GROUPED
    // column block tile_n of the launch is block tile_n % bpm of member tile_n / bpm: from here on the tile is that member's alone
    const int member = tile_n / g_.bpm;
    tile_n -= member * g_.bpm;
    const uint8_t* const w = g_.slab[member];
#endif
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
#if AQ_GROUPED
    // the member's scales, bias and output matrix ([M][N] at element offset M N member of the launch's one buffer) stand in for the launch's
    const float* const t_sb = g_.sb[member];
    const void* const t_bias = g_.bias[member];
    uint8_t* const t_out = (uint8_t*)p_.out + (int64_t)M * N * member * 2;
    const int64_t t_ldc = N;
    SDNQ_KERNARGS_NOW("s"(t_sb), "s"(t_bias), "s"(p_.out), "s"(p_.bias_dtype), "s"(p_.trace));
#define AQ_SB t_sb
#define AQ_BIAS t_bias
#define AQ_OUT t_out
#define AQ_LDC t_ldc
#else
    SDNQ_KERNARGS_NOW("s"(p_.sb), "s"(p_.bias), "s"(p_.out), "s"(p_.ldc), "s"(p_.bias_dtype), "s"(p_.trace));
#define AQ_SB p.sb
#define AQ_BIAS p.bias
#define AQ_OUT (uint8_t*)p.out
#define AQ_LDC p.ldc
#endif
    if (p.trace != nullptr && tid == 0 && blockIdx.x < 1024) p.trace[blockIdx.x * 8] = t_entry;
    SDNQ_PHASE_STAMP(p.trace, 1);
    // per-channel epilogue vectors: requested now (behind the rows and the ring prologue), parked in LDS after the quantization
    float ev_sb = 0.0f;
    u32 ev_bias = 0;  // raw bits: converted when parked (a conversion here would wait for every load in flight)
    if (tid < BN) {
        const int64_t gi = n0 + (tid < n_lim ? tid : n_lim - 1);
        ev_sb = AQ_SB[gi];
        if constexpr (HAS_BIAS) {
            if (p.bias_dtype == SDNQ_F32) ev_bias = ((const u32*)AQ_BIAS)[gi];
            else ev_bias = ((const uint16_t*)AQ_BIAS)[gi];
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
    // A wave holds ONE 32 x 32 accumulator.  Its zeroing here and the epilogue below stand in a loop of one trip over the wave's blocks:
    // written without the loop statement, the 64 x 128 kernels come out with a branch and a register allocated differently
    // (tools/compare_kernels.py), and this kernel's code is kept as measured.
    typename MT::acc_t acc;
#pragma unroll
    for (int blk = 0; blk < 1; ++blk)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0;
    const int wm = wave / (BN / 32), wn = wave % (BN / 32);  // 32-row block, 32-column block of the wave
    const int frow = lane & 31, fgrp = lane >> 5;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's codes and scales are in LDS before the first barrier lets anyone read them
    typename MT::frag_t fa[2][KS];
    if constexpr (DIRECT) {
        // Direct form: the slab loop below with the weight fragments already in registers.  Sub-step ks of stage kt multiplies
        // fbd[kt % RD][ks] as soon as that load has landed, and the register is reloaded with the same sub-step of stage kt + RD.
        auto read_a = [&](auto setc, auto ksc, int st) {
            constexpr int sx = decltype(setc)::value, ks = decltype(ksc)::value;
            fa[sx][ks] = MT::load(ldsA + (st < nk ? st : 0) * A_STAGE, wm * 32 + frow, ks, fgrp);
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
                    MT::mma(acc, fbd[slot][ks], fa[sx][ks]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (kt + 1 < NJ) read_a(std::integral_constant<int, sx ^ 1>{}, ksc, kt + 1);
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
            fa[sx][ks] = MT::load(ldsA + (st < nk ? st : 0) * A_STAGE, wm * 32 + frow, ks, fgrp);
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
                    MT::mma(acc, kt < DF ? fbr[kt < DF ? kt : 0][ks] : fbs[ks], fa[sx][ks]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (kt + 1 < NJ) read_a(std::integral_constant<int, sx ^ 1>{}, ksc, kt + 1);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    } else {
        // Software pipeline one STAGE deep (the whole-stage overlapped ring of profiles/r05_overlapped_ring_lab.txt): the fragments of stage kt sit in
        // registers when its barrier falls, so the MFMAs start at once; dealt out between them are the fragment reads of stage kt + 1 (which that
        // barrier published) and the DMA pieces of stage kt + NSB into the slot stage kt has just vacated -- NSB - 1 stages in flight behind the
        // landed one.  Two register sets, so the loop is unrolled by two.
        typename MT::frag_t fb[2][KS];
        auto read_stage = [&](auto setc, auto ksc, int st, int slot) {
            constexpr int sx = decltype(setc)::value, ks = decltype(ksc)::value;
            fa[sx][ks] = MT::load(ldsA + (st < nk ? st : 0) * A_STAGE, wm * 32 + frow, ks, fgrp);
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
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            const int slot_free = slot_c;
            slot_c = (slot_c + 1 == NSB) ? 0 : slot_c + 1;
            // MFMA ks of stage kt, then read ks of stage kt + 1 (the last sub-step's reads retire under the next barrier's wait; KS <= 4)
            static_for_up<KS>([&](auto ksc) {
                constexpr int ks = decltype(ksc)::value;
                MT::mma(acc, fb[sx][ks], fa[sx][ks]);
                __builtin_amdgcn_sched_barrier(0);
                read_stage(std::integral_constant<int, sx ^ 1>{}, ksc, kt + 1, slot_c);
                if constexpr (ks == 0) issueB(kt + NSB, slot_free);
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
    for (int blk = 0; blk < 1; ++blk) {  // (one block; the loop statement is kept for the reason given at the accumulator above)
        const int ml = wm * 32 + frow;
        const float sa = s_xs[ml];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nl0 = wn * 32 + 8 * q + 4 * fgrp;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float vv = MT::tof(acc, 4 * q + e) * sa;
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
                                    (v4i*)(AQ_OUT + ((int64_t)(m0 + r) * AQ_LDC + n0 + c * 8) * 2));
    }
    SDNQ_PHASE_STAMP(p.trace, 6);
}
#undef AQ_SB
#undef AQ_BIAS
#undef AQ_OUT
#undef AQ_LDC
