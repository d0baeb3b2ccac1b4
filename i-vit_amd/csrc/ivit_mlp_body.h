// ivit_mlp_body.h — the body of the lock-step fused-Mlp kernel (the scheme: ivit_mlp.h).  Not a header of its own: ivit_mlp.h includes it
// once inside each entry point (mlp384_kernel, mlp256_kernel, mlp192_kernel, mlp128_body and the LayerNorm-headed mlp384ln_kernel,
// mlp192ln_kernel), which supplies `G` (the geometry), `FMA` (the requant form: rq_magic), `LNH` (the activation tile of a unit is norm2 +
// qact3 of its rows of the 16-bit stream, computed in place: below) and `p` (MlpArgs).  One
// text, so that a change to the barriers, the prefetch distances or ShiftGELU reaches every width; included rather than called,
// so that each entry point compiles exactly as if the body were written out in it.
    extern __shared__ __attribute__((aligned(256))) char sm[];
    constexpr int NJ = G::NJ;                       // channel tiles per step
    constexpr int CT1 = G::HD / 16 / G::WAVES;      // channel tiles of fc1 per wave, in chunks of NJ
    constexpr int NCH = CT1 / NJ, NS1 = NCH * G::KS1, WD = G::WD;   // fc1 chunks, fc1 steps, weight prefetch distance
    constexpr int ACH = G::C / 16;                  // 16-byte chunks of an activation row
    constexpr int AREG = (G::TT * 16 * ACH + G::THREADS - 1) / G::THREADS;
    static_assert(NJ * 16 * G::WAVES == G::C && CT1 % NJ == 0, "wave count must split the channel tiles of fc1 and fc2 evenly");
    // (the two may share a step: the multipliers are requested in the step's first fenced region, the bias — after the step has
    // copied the current one into its accumulators — in the second, so the multipliers still come back first)
    static_assert(G::KS1 >= 2 && G::CQ_STEP <= G::BIAS_STEP && G::BIAS_STEP < G::KS1 - 1,
                  "the fc1 pipeline loads a chunk's multipliers, then the next bias, both before the chunk's last step");
    static_assert(G::WG_PER_CU * (LNH ? G::SMEM_LN : G::SMEM) <= 160 * 1024, "WG_PER_CU workgroups share a CU's LDS");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // G::DIRECT: four channels' (m, 2^-e) pairs as the caller's table holds them -> their multipliers c = m * 2^-e
    auto dy_c = [](const v2d (&d)[4], v2d (&c)[2]) __attribute__((always_inline)) {
        c[0] = v2d{d[0][0] * d[0][1], d[1][0] * d[1][1]};
        c[1] = v2d{d[2][0] * d[2][1], d[3][0] * d[3][1]};
    };

    // ---- this workgroup's units: (first tile, tiles) of unit i
    MLP_UNIT_SCHEDULE(G::TT, G::ROUND_ROBIN);

    // activation tile of a unit (rows x ACH chunks of 16 B): global -> registers (a_fetch), registers -> LDS (a_commit).  With
    // G::OPAQUE_A, row and chunk of a lane come from an opaque copy of the thread id
    v4i areg[AREG];
    auto a_fetch = [&](long long tile0, int ntt) __attribute__((always_inline)) {
        int t = threadIdx.x;
        if constexpr (G::OPAQUE_A) asm volatile("" : "+v"(t));
#pragma unroll
        for (int i = 0; i < AREG; ++i) {
            const int ch = t + i * G::THREADS, row = ch / ACH, c16 = ch - row * ACH;
            if (ch < ntt * 16 * ACH) {
                const long long grow = min(tile0 * 16 + row, p.M - 1);
                areg[i] = *reinterpret_cast<const v4i *>(p.x + grow * G::C + c16 * 16);
            }
        }
    };
    auto a_commit = [&](int ntt) __attribute__((always_inline)) {
        int t = threadIdx.x;
        if constexpr (G::OPAQUE_A) asm volatile("" : "+v"(t));
#pragma unroll
        for (int i = 0; i < AREG; ++i) {
            const int ch = t + i * G::THREADS, row = ch / ACH, c16 = ch - row * ACH;
            if (ch < ntt * 16 * ACH)
                *reinterpret_cast<v4i *>(sm + G::SA + (c16 >> 2) * G::KBLK + row * 64 + mlp_phi(row, c16 & 3) * 16) = areg[i];
        }
    };

    // LNH: the tile is not copied from p.x but computed — norm2 + qact3 (vit_quant.py:139-140) of the unit's rows of p.residual, the
    // 16-bit stream that is LayerNorm input AND identity branch — so the LayerNorm's bytes never exist in HBM.  The arithmetic is
    // LnGroup<C, 2> (8 lanes per row, 8 rows per wave and pass: layernorm_reg_kernel's, byte for byte); lane (k, h) of a row owns
    // channels 32 i + 8 k + 4 h .. + 3 of step i, i.e. 4 bytes of chunk (i & 1) * 2 + (k >> 1) of K block i >> 1, stored where a_commit
    // puts that (row, chunk).  Rows >= M are row M - 1 again (as a_fetch clamps them): the tile holds defined bytes.  The per-channel
    // constants live behind the table lines at 16 B per channel (c fp64, bias_int, sc: what fits beside two workgroups per CU at
    // width 192 and one at 384), so 1 / sc is formed per element (LnGroup::run<.., LOCAL_Y>).  ln_fetch requests the 16-bit rows of
    // one pass (in front of ShiftGELU for a unit's first pass, one pass ahead after that), ln_rows normalises them into the tile
    typedef LnGroup<G::C, 2> LG;
    typedef typename LG::Raw ln_raw;
    double *const cC = reinterpret_cast<double *>(sm + G::SLN);
    float *const cB = reinterpret_cast<float *>(sm + G::SLN + G::C * 8), *const cSc = cB + G::C;
    bool ln_fast = false;
    // (the vote of ln_stage_constants goes through the first word of the table lines: nothing writes those before barrier B2 of unit 0)
    if constexpr (LNH)
        ln_fast = ln_stage_constants<G::C, G::THREADS, false>(p.ln_bias_int, p.ln_sc, p.ln_dy, cC, cB, cSc, reinterpret_cast<float *>(sm + G::STAB));
    auto ln_fetch = [&](ln_raw (&raw)[LG::NSTEP], long long tile0, int r0) __attribute__((always_inline)) {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const int j = t & 7;
        const long long grow = min(tile0 * 16 + r0 + ((t & 63) >> 3), p.M - 1);
        const int16_t *xp = p.residual + grow * G::C + 4 * j;           // 8 k + 4 h with j = 2 k + h
#pragma unroll
        for (int i = 0; i < LG::NSTEP; ++i) raw[i] = *reinterpret_cast<const ln_raw *>(xp + 32 * i);
    };
    auto ln_rows = [&](const ln_raw (&raw)[LG::NSTEP], int r0) __attribute__((always_inline)) {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const int j = t & 7, k = j >> 1, row = r0 + ((t & 63) >> 3);
        const float ys = rcp_rn(p.ln_s);
        float xv[LG::NSTEP][LG::EPC];
        LN_ROW_X(LG, xv, raw[i], p.ln_s, ys);
        char *const rowa = sm + G::SA + row * 64 + (k & 1) * 8 + 4 * (j & 1);
        const int ph0 = mlp_phi(row, k >> 1) * 16, ph1 = mlp_phi(row, 2 + (k >> 1)) * 16;
        auto place = [&](int i, unsigned pk0, unsigned) __attribute__((always_inline)) {
            *reinterpret_cast<unsigned *>(rowa + (i >> 1) * G::KBLK + ((i & 1) ? ph1 : ph0)) = pk0;
        };
        LG::template run<std::false_type, decltype(place), true>(xv, j, k, 4 * j, ln_fast, true, cC, cB, cSc, nullptr, place);
    };
    // the passes of a unit's tile behind the first fetch: rows r0, r0 + 8 WAVES, ... of this wave
    auto ln_tile = [&](ln_raw (&raw)[LG::NSTEP], long long tile0, int ntt) __attribute__((always_inline)) {
        for (int r0 = wave * 8; r0 < ntt * 16; r0 += G::WAVES * 8) {
            ln_raw cur[LG::NSTEP];
#pragma unroll
            for (int i = 0; i < LG::NSTEP; ++i) cur[i] = raw[i];
            if (r0 + G::WAVES * 8 < ntt * 16) ln_fetch(raw, tile0, r0 + G::WAVES * 8);
            ln_rows(cur, r0);
        }
    };
    ln_raw lraw[LG::NSTEP];

    // ------------------------------------------------------------------------------------------------------------------
    // one unit of NTT token tiles starting at tile `tile0`; (next_tile0, next_ntt): the unit whose activations to prefetch
    // Barriers: B1 before the first hidden write (every wave is done reading the previous unit's hidden tile; placed AFTER the
    // first chunk's K loop, so a wave that finished its fc2 early already multiplies for the next unit), B2 hidden tile
    // complete / activation tile dead, B3 hidden tile rewritten by ShiftGELU and the NEXT unit's activation tile committed.
    auto unit_body = [&](auto ntt_c, const int ntt, const long long tile0, const long long next_tile0, const int next_ntt) __attribute__((always_inline)) {
        constexpr int NTT = decltype(ntt_c)::value;       // tiles the body multiplies; `ntt` <= NTT of them belong to this unit
        const long long tok0 = tile0 * 16;
        // per-lane indices from an opaque copy of the thread id: every LDS address below is (a handful of per-lane bases) +
        // immediates, recomputed per unit — left visible, the ~150 loop-invariant addresses of the unrolled phases are
        // hoisted out of the unit loop into registers and spilled
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, tl = lane & 15, g = lane >> 4;
        const unsigned fb = tl * 64 + mlp_phi(tl, g) * 16;          // this lane's B-fragment chunk inside a K block, token tile 0

        // ---- fc1 + qact_gelu (8 bit) into the hidden tile
        {
            const v4i *w1 = p.w1f + (size_t)(wave * NJ) * 64 + lane;
            // G::DIRECT: this lane's 16 bytes of the fragment (this wave's first channel tile, column step 0) of the row-major W1 [HD][C];
            // every other fragment of the wave is a compile-time offset from it
            const int8_t *w1d = reinterpret_cast<const int8_t *>(p.w1f) + (wave * CT1 * 16 + tl) * G::C + g * 16;
            v4i wf[WD + 1][NJ], bf[2][NTT], acc[NJ][NTT], bias_n[NJ];
            v2d cq[NJ][2], dq[G::DIRECT ? NJ : 1][4];
            auto load_w = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if constexpr (G::DIRECT)
                        wf[slot][j] = *reinterpret_cast<const v4i *>(w1d + (((s / G::KS1) * NJ + j) * 16) * G::C + (s % G::KS1) * 64);
                    else wf[slot][j] = w1[(size_t)(s * NJ * G::WAVES + j) * 64];
                }
            };
            auto load_b = [&](int s, int slot) __attribute__((always_inline)) {
                const int ks = s % G::KS1;
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt)
                    bf[slot][tt] = *reinterpret_cast<const v4i *>(sm + G::SA + ks * G::KBLK + tt * 1024 + fb);
            };
            auto load_bias = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if (G::DIRECT && !p.b1) bias_n[j] = v4i{0, 0, 0, 0};
                    else bias_n[j] = *reinterpret_cast<const v4i *>(p.b1 + (wave * CT1 + chunk * NJ + j) * 16 + 4 * g);
                }
            };
#pragma unroll
            for (int s = 0; s < WD; ++s) load_w(s, s);
            load_b(0, 0);
            load_bias(0);
#pragma unroll
            for (int s = 0; s < NS1; ++s) {
                const int chunk = s / G::KS1, ks = s - chunk * G::KS1, ct0 = wave * CT1 + chunk * NJ;
                __builtin_amdgcn_sched_barrier(0);
                if (s + WD < NS1) load_w(s + WD, (s + WD) % (WD + 1));
                if (s + 1 < NS1) load_b(s + 1, (s + 1) & 1);
                if (ks == G::CQ_STEP) {              // this chunk's multipliers: consumed at its last step
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int ch0 = (ct0 + j) * 16 + 4 * g;
                        if constexpr (G::DIRECT) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) dq[j][e] = reinterpret_cast<const v2d *>(p.cq1)[ch0 + e];
                        } else {
                            cq[j][0] = *reinterpret_cast<const v2d *>(p.cq1 + ch0);
                            cq[j][1] = *reinterpret_cast<const v2d *>(p.cq1 + ch0 + 2);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ks == 0) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int tt = 0; tt < NTT; ++tt) acc[j][tt] = bias_n[j];
                }
                if (ks == G::BIAS_STEP && chunk + 1 < NCH) load_bias(chunk + 1);      // the next chunk's bias, consumed at its first step
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int tt = 0; tt < NTT; ++tt)
                        acc[j][tt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[s % (WD + 1)][j], bf[s & 1][tt], acc[j][tt], 0, 0, 0);
                if (ks == G::KS1 - 1) {
                    if (chunk == 0) __syncthreads();                       // B1: the hidden tile is free
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        if constexpr (G::DIRECT) dy_c(dq[j], cq[j]);
                        const int ch0 = (ct0 + j) * 16 + 4 * g;               // this lane's 4 hidden channels
                        const int kb = ch0 >> 6, cc = (ch0 >> 4) & 3;           // fc2 K block and chunk of these channels
#pragma unroll
                        for (int tt = 0; tt < NTT; ++tt) {
                            int o[4];
                            o[0] = rq_magic<FMA>(acc[j][tt][0], cq[j][0][0]);
                            o[1] = rq_magic<FMA>(acc[j][tt][1], cq[j][0][1]);
                            o[2] = rq_magic<FMA>(acc[j][tt][2], cq[j][1][0]);
                            o[3] = rq_magic<FMA>(acc[j][tt][3], cq[j][1][1]);
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] = min(max(o[e], -128), 127);
                            const unsigned w01 = __builtin_amdgcn_perm((unsigned)o[1], (unsigned)o[0], 0x0c0c0400u);
                            const unsigned w23 = __builtin_amdgcn_perm((unsigned)o[3], (unsigned)o[2], 0x0c0c0400u);
                            const int tok = tt * 16 + tl;
                            *reinterpret_cast<unsigned *>(sm + G::SH + kb * G::KBLK + tok * 64 + mlp_phi(tok, cc) * 16 + 4 * g) =
                                __builtin_amdgcn_perm(w23, w01, 0x05040100u);
                        }
                    }
                }
            }
        }
        __syncthreads();                                                    // B2

        // ---- ShiftGELU (+ qact1) in place, half a wavefront per token, NTOK tokens per half-wave: the token's HD hidden
        // bytes are read once (NW dwords per lane) and stay in registers from the row maximum (packed byte maxima, then 5
        // shuffles) over the fetch of the maximum's 256-byte table line (global -> this half-wave's LDS slot) to the byte
        // gathers and the write-back.  No workgroup barrier inside.  The next unit's activations travel meanwhile.
        if constexpr (LNH) {
            if (wave * 8 < next_ntt * 16) ln_fetch(lraw, next_tile0, wave * 8);
        } else if (next_ntt > 0) a_fetch(next_tile0, next_ntt);
        {
            const int hw = wave * 2 + (lane >> 5), l32 = lane & 31;
            typedef unsigned short v2us __attribute__((ext_vector_type(2)));
            const unsigned sm_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char *)sm;
            const unsigned base = sm_lds + G::STAB + hw * 256;           // 256-byte aligned: byte | base is the address
            constexpr int NW = G::KS2 / 2;                                           // dwords of a hidden row per lane
            constexpr int NTOK = (NTT * 16 + 2 * G::WAVES - 1) / (2 * G::WAVES);     // tokens per half-wave
            unsigned w[NTOK][NW];
            v2i line[NTOK];
            // pass 1: rows -> registers, row maxima, all table-line requests in flight together (one exposed L2 latency
            // per unit instead of one per token)
#pragma unroll
            for (int i = 0; i < NTOK; ++i) {
                const int t = hw + i * 2 * G::WAVES;
                if (t < NTT * 16) {
                    const unsigned *hp = reinterpret_cast<const unsigned *>(sm + G::SH + t * 64) + (l32 & 15) + (l32 >> 4) * (G::KBLK / 4);
                    v2us me = {0, 0}, mo = {0, 0};                          // running maxima of the even / odd bytes (biased)
#pragma unroll
                    for (int m = 0; m < NW; ++m) {
                        w[i][m] = hp[m * (G::KBLK / 2)] ^ 0x80808080u;     // K blocks 2m, 2m + 1 (the upper 16 lanes): Q + 128
                        me = __builtin_elementwise_max(me, __builtin_bit_cast(v2us, __builtin_amdgcn_perm(0u, w[i][m], 0x0c020c00u)));
                        mo = __builtin_elementwise_max(mo, __builtin_bit_cast(v2us, __builtin_amdgcn_perm(0u, w[i][m], 0x0c030c01u)));
                    }
                    const v2us m2 = __builtin_elementwise_max(me, mo);
                    int qb = max((int)m2[0], (int)m2[1]);                    // biased row maximum of this lane
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) qb = max(qb, __shfl_xor(qb, o));
                    line[i] = reinterpret_cast<const v2i *>(p.tab + (size_t)qb * 256)[l32];
                }
            }
            // pass 2: table line -> this half-wave's LDS slot, byte gathers, write-back.  Wave-level ordering only: the slot
            // belongs to this half-wave and the previous token's gathers were consumed by its write-back
#pragma unroll
            for (int i = 0; i < NTOK; ++i) {
                const int t = hw + i * 2 * G::WAVES;
                if (t < NTT * 16) {
                    unsigned *hp = reinterpret_cast<unsigned *>(sm + G::SH + t * 64) + (l32 & 15) + (l32 >> 4) * (G::KBLK / 4);
                    reinterpret_cast<v2i *>(sm + G::STAB + hw * 256)[l32] = line[i];
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
                    for (int m = 0; m < NW; ++m) {
                        const unsigned x = w[i][m];
                        const unsigned b0 = *(lds_u8 *)(size_t)(base | (x & 0xffu)), b1 = *(lds_u8 *)(size_t)(base | ((x >> 8) & 0xffu));
                        const unsigned b2 = *(lds_u8 *)(size_t)(base | ((x >> 16) & 0xffu)), b3 = *(lds_u8 *)(size_t)(base | (x >> 24));
                        hp[m * (G::KBLK / 2)] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
                    }
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
            }
        }
        if constexpr (LNH) ln_tile(lraw, next_tile0, next_ntt);
        else if (next_ntt > 0) a_commit(next_ntt);
        __syncthreads();                                                    // B3

        // ---- fc2 + qact2 (16 bit) + qact4 with the identity branch (16 bit)
        {
            const v4i *w2 = p.w2f + (size_t)(wave * NJ) * 64 + lane;
            const int8_t *w2d = reinterpret_cast<const int8_t *>(p.w2f) + (wave * NJ * 16 + tl) * G::HD + g * 16;      // G::DIRECT: as w1d, of W2 [C][HD]
            v4i wf[WD + 1][NJ], bf[2][NTT], acc[NJ][NTT];
            auto load_w = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if constexpr (G::DIRECT) wf[slot][j] = *reinterpret_cast<const v4i *>(w2d + (j * 16) * G::HD + s * 64);
                    else wf[slot][j] = w2[(size_t)(s * NJ * G::WAVES + j) * 64];
                }
            };
            auto load_b = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt)
                    bf[slot][tt] = *reinterpret_cast<const v4i *>(sm + G::SH + s * G::KBLK + tt * 1024 + fb);
            };
#pragma unroll
            for (int s = 0; s < WD; ++s) load_w(s, s);
            load_b(0, 0);
            // identity rows and multipliers of this lane's outputs: requested now, consumed after the K loop (G::DIRECT: the multipliers
            // are read and formed after the loop, from L2-resident tables: the form that was measured)
            v2i rs[NJ][NTT];
            v2d c2[NJ][2];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ch0 = (wave * NJ + j) * 16 + 4 * g;
                if constexpr (!G::DIRECT) {
                    c2[j][0] = *reinterpret_cast<const v2d *>(p.cq2 + ch0);
                    c2[j][1] = *reinterpret_cast<const v2d *>(p.cq2 + ch0 + 2);
                }
                const v4i b4 = (G::DIRECT && !p.b2) ? v4i{0, 0, 0, 0} : *reinterpret_cast<const v4i *>(p.b2 + ch0);
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt) {
                    acc[j][tt] = b4;
                    const long long tok = min(tok0 + tt * 16 + tl, p.M - 1);
                    rs[j][tt] = *reinterpret_cast<const v2i *>(p.residual + tok * G::C + ch0);
                }
            }
#pragma unroll
            for (int s = 0; s < G::KS2; ++s) {
                __builtin_amdgcn_sched_barrier(0);
                if (s + WD < G::KS2) load_w(s + WD, (s + WD) % (WD + 1));
                if (s + 1 < G::KS2) load_b(s + 1, (s + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int tt = 0; tt < NTT; ++tt)
                        acc[j][tt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[s % (WD + 1)][j], bf[s & 1][tt], acc[j][tt], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ch0 = (wave * NJ + j) * 16 + 4 * g;
                if constexpr (G::DIRECT) {
                    v2d d[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = reinterpret_cast<const v2d *>(p.cq2)[ch0 + e];
                    dy_c(d, c2[j]);
                }
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt) {
                    int t16[4];
                    t16[0] = rq_magic<FMA>(acc[j][tt][0], c2[j][0][0]);
                    t16[1] = rq_magic<FMA>(acc[j][tt][1], c2[j][0][1]);
                    t16[2] = rq_magic<FMA>(acc[j][tt][2], c2[j][1][0]);
                    t16[3] = rq_magic<FMA>(acc[j][tt][3], c2[j][1][1]);
                    int o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = min(max(t16[e], -32768), 32767);
                        const int r = (int)(short)((unsigned)rs[j][tt][e >> 1] >> (16 * (e & 1)));
                        // both terms are integers < 2^31: the sum is the reference's fp64 sum (quant_utils.py:238-244)
                        o[e] = min(max(rq_fast(r, p.cr) + rq_fast(t, p.cm), -32768), 32767);
                    }
                    const long long tok = tok0 + tt * 16 + tl;
                    if (tok < p.M && tt < ntt)         // a short unit's surplus tiles belong to the next unit
                        *reinterpret_cast<v2i *>(p.out + tok * G::C + ch0) =
                            v2i{(int)__builtin_amdgcn_perm((unsigned)o[1], (unsigned)o[0], 0x05040100u),
                                (int)__builtin_amdgcn_perm((unsigned)o[3], (unsigned)o[2], 0x05040100u)};
                }
            }
        }
    };

    // ---- the unit stream
    if constexpr (LNH) {
        if (wave * 8 < unit_ntt(0) * 16) ln_fetch(lraw, unit_tile0(0), wave * 8);
        ln_tile(lraw, unit_tile0(0), unit_ntt(0));
    } else {
        a_fetch(unit_tile0(0), unit_ntt(0));
        a_commit(unit_ntt(0));
    }
    __syncthreads();
    for (int i = 0; i < nu; ++i) {
        const long long tile0 = unit_tile0(i), tile1 = unit_tile0(i + 1);
        const int ntt = unit_ntt(i), next_ntt = unit_ntt(i + 1);
        if (ntt == G::TT) unit_body(std::integral_constant<int, G::TT>{}, ntt, tile0, tile1, next_ntt);
        else unit_body(std::integral_constant<int, G::TT - 1>{}, ntt, tile0, tile1, next_ntt);
    }

