// sgr_res_body.h -- the body of the resident self-guided search kernels (lr_search.hip), included once per instance:
// sgr_res_kernel<T, TREE> (every item) and sgr_res_small_kernel<T> (small one-part items).  Textual inclusion, not a
// __device__ template: wrapped in an always-inline function the big instance, which sits at the edge of its 128-VGPR
// budget, was allocated differently and spilled 42 VGPRs in its load phase (0 as a kernel body).
// The including kernel defines, besides its parameters (A, nplanes, items, cfg, nodes_arg, ds, xch, xmode, status,
// stat, tk) and T / TREE:
//   KMAX  the instance's chunk capacity per lane -- g (4 KMAX VGPRs), the LDS size (sr_lds_bytes) and sr_pass's
//         unroll follow it
//   ONE   an instance of one-part items on the default one-barrier path only: the row-part exchange and the
//         two-barrier loops are not compiled in
    PROF_BEGIN(tk);
    // one node per pass in the default kernel: a compile-time constant there, so the per-lane tree builder (a
    // divergent Descent copy per lane) is not compiled in and the descent keeps to registers
    const int nodes = TREE ? nodes_arg : 1;
    // [half][chunk k][pixel lane]: (x - src) of pixels 0, 1 (half 0) and 2, 3 (half 1), int16 pairs -- two planes of
    // lane-linear words, the layout the direct global -> LDS loads (SVTGPU_SR_GLDS) write
    extern __shared__ uint32_t sr_dx[];
    // wave partials: the moments, then each pass's errors; two buffers by pass parity (the one-barrier path of
    // one-part items reads a pass's partials while the next pass writes the other buffer)
    __shared__ unsigned long long s_red2[2][SR_PW][SG_NC];
    unsigned long long (*const s_red)[SG_NC] = s_red2[0];
    // one-barrier path: the seeded descent every wave steps itself (raw storage: Descent has member initializers)
    __shared__ __attribute__((aligned(8))) unsigned char s_desc_raw[sizeof(Descent)];
    Descent &s_desc = *reinterpret_cast<Descent *>(s_desc_raw);
    __shared__ unsigned long long s_etot[2]; // self-stepping row parts: each pass's error summed over the parts
    __shared__ int                s_xok[2];  // ... and whether the exchange succeeded
    __shared__ uint32_t           s_xq[SG_NC];         // the pending tree's candidates (xq pairs), compacted
    __shared__ uint32_t           s_mask;              // its nodes
    __shared__ int                s_nv;                // its candidate count (0: the descent has ended)
    const SrItem it = items[blockIdx.x];
    if (it.pair < 0) return; // an empty slot of the XCD-ordered grid (uniform)
    int p = 0;
    while (p + 1 < nplanes && it.pair >= A.pl[p + 1].pair_base) p++;
    const PlaneArgs &P  = A.pl[p];
    const int        ul = (it.pair - P.pair_base) / P.ne, k = it.pair - P.pair_base - ul * P.ne, ep = P.eps[k];
    const URect      ur = A.units[P.unit_base + ul];
    const int        uw = ur.h_end - ur.h_start, cw = (uw + 3) >> 2, nch = cw * (it.y1 - it.y0), K = (nch + SR_PL - 1) / SR_PL;
    // the host plans parts that fit the instance (and only one-part items for a ONE instance); never index past the
    // registers
    if (K > KMAX || nch <= 0 || (ONE && it.nparts != 1)) {
        if (threadIdx.x == 0) atomicOr(status, 4);
        return;
    }
    // the wave's role from a scalar (readfirstlane) condition: the compiler then treats each role's code as uniform
    // control flow -- with `threadIdx.x < SR_PL` it could not prove the branch wave-uniform and compiled the control
    // wave's descent steps as exec-masked vector code with scratch traffic
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) < SR_PW) {
        // ================= pixel waves =================
        const int      pl = threadIdx.x, r0 = c_sgr_r[ep][0], r1 = c_sgr_r[ep][1];
        const T       *d = (const T *)P.dgd, *s = (const T *)P.src;
        const size_t   pn = (size_t)P.fstride * P.H;
        // an ep without one of the filters reads a plane that holds no data: its g half is zeroed
        const int16_t *f0 = P.flt + (size_t)k * 2 * pn, *f1 = P.flt + (size_t)P.f1e[k] * 2 * pn + pn;
        const uint32_t gmask = (r0 ? 0x0000FFFFu : 0u) | (r1 ? 0xFFFF0000u : 0u);
        // ---- load the part: g in registers, (x - src) in LDS, the moments on the way ----
        // Chunk kk of this lane is chunk c = pl + kk * SR_PL of the part (row-major over 4-sample columns); its
        // (row, column) advance by a fixed step from one kk to the next (no division per chunk).  Chunks past the part
        // read the part's last chunk (addresses stay inside) and contribute zeros.
        const int      dr = SR_PL / cw, dc = SR_PL - dr * cw, lastc = nch - 1, lrow = lastc / cw, lcol = lastc - lrow * cw;
        int            crow = pl / cw, ccol = pl - crow * cw; // chunk 0 of this lane
        auto           chunk_at = [&](int kk, int &row, int &col) {   // (row, col) of chunk kk, clamped into the part
            row = crow, col = ccol;
            if (pl + kk * SR_PL >= nch) row = lrow, col = lcol;
        };
        auto           advance = [&]() {
            crow += dr, ccol += dc;
            if (ccol >= cw) ccol -= cw, crow++;
        };
        // 1. the ep's two filter planes of every chunk, straight into g (raw int16 pairs: flt0 of pixels 0, 1 | 2, 3
        //    then flt1 of them): every HBM read of the part in flight at once, one memory round trip per item
        uint32_t g[KMAX][4];
#pragma unroll
        for (int kk = 0; kk < KMAX; kk++) {
            g[kk][0] = g[kk][1] = g[kk][2] = g[kk][3] = 0u;
            if (kk < K) { // uniform
                int row, col;
                chunk_at(kk, row, col);
                const size_t fo = (size_t)(ur.v_start + it.y0 + row) * P.fstride + ur.h_start + 4 * col;
                // an ep without one of the filters (eps 10-15) reads only the other plane (r0 / r1 uniform)
                const uint2  a0 = r0 ? *(const uint2 *)(f0 + fo) : make_uint2(0u, 0u);
                const uint2  a1 = r1 ? *(const uint2 *)(f1 + fo) : make_uint2(0u, 0u);
                g[kk][0] = a0.x, g[kk][1] = a0.y, g[kk][2] = a1.x, g[kk][3] = a1.y;
                advance();
            }
        }
        // 2. dx = dgd - src (the plane unit_sums_kernel writes; the eps of a unit read it through one L2) in groups of
        //    SR_LB chunks: the moments, and the (x - src) pairs to LDS.  g (1.) already holds flt - (dgd << 4), so a
        //    chunk needs two registers here instead of four for the CDEF output and the source: half the round trips
        crow = pl / cw, ccol = pl - crow * cw;
        unsigned long long M0 = 0, M1 = 0, M2 = 0, M3 = 0, M4 = 0; // M2..M4 hold signed sums mod 2^64
#if SVTGPU_SR_GLDS
        // every chunk's dx straight into its LDS words with direct global -> LDS loads (no registers: one round trip
        // for the part), then each lane reads its own words back, masks them and forms the moments
        {
            uint32_t *lw = sr_dx + (pl & ~63); // the wave's lane-linear base: lane l of the wave lands at lw[l + ...]
#pragma unroll
            for (int kk = 0; kk < KMAX; kk++) {
                if (kk >= K) break; // uniform
                int row, col;
                chunk_at(kk, row, col);
                const int16_t *src = P.dxp + (size_t)(ur.v_start + it.y0 + row) * P.fstride + ur.h_start + 4 * col;
                __builtin_amdgcn_global_load_lds((const void *)src,
                                                 (__attribute__((address_space(3))) void *)(lw + kk * SR_PL), 4, 0, 0);
                __builtin_amdgcn_global_load_lds((const void *)(src + 2),
                                                 (__attribute__((address_space(3))) void *)(lw + (KMAX + kk) * SR_PL),
                                                 4, 0, 0);
                advance();
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        crow = pl / cw, ccol = pl - crow * cw;
#pragma unroll
        for (int kk = 0; kk < KMAX; kk++) {
            if (kk >= K) { // uniform: zeros up to the next multiple of SR_LB (sr_pass reads whole groups)
                if (kk < ((K + SR_LB - 1) & ~(SR_LB - 1))) sr_dx[kk * SR_PL + pl] = sr_dx[(KMAX + kk) * SR_PL + pl] = 0u;
                continue;
            }
            int row, col;
            chunk_at(kk, row, col);
            const int nin = pl + kk * SR_PL < nch ? min(4, uw - 4 * col) : 0;
            advance();
            const uint32_t mlo = nin >= 2 ? ~0u : nin == 1 ? 0xFFFFu : 0u;
            const uint32_t mhi = nin >= 4 ? ~0u : nin == 3 ? 0xFFFFu : 0u;
            g[kk][0] &= mlo, g[kk][2] &= mlo, g[kk][1] &= mhi, g[kk][3] &= mhi;
            const uint2 x2 = make_uint2(sr_dx[kk * SR_PL + pl] & mlo, sr_dx[(KMAX + kk) * SR_PL + pl] & mhi);
            if (nin < 4) sr_dx[kk * SR_PL + pl] = x2.x, sr_dx[(KMAX + kk) * SR_PL + pl] = x2.y;
            const int      dxq[4] = {(int)(int16_t)(x2.x & 0xFFFF), (int)x2.x >> 16, (int)(int16_t)(x2.y & 0xFFFF),
                                     (int)x2.y >> 16};
            const uint32_t fw[4] = {__builtin_amdgcn_perm(g[kk][2], g[kk][0], 0x05040100u),
                                    __builtin_amdgcn_perm(g[kk][2], g[kk][0], 0x07060302u),
                                    __builtin_amdgcn_perm(g[kk][3], g[kk][1], 0x05040100u),
                                    __builtin_amdgcn_perm(g[kk][3], g[kk][1], 0x07060302u)};
            uint32_t m0 = 0, m1 = 0;
            int      m3 = 0, m4 = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t gq = fw[q] & gmask;
                const int      g1 = (int)(int16_t)(gq & 0xFFFF), g2 = (int)gq >> 16, ss = -(dxq[q] << 4);
                m0 += (uint32_t)(g1 * g1), m1 += (uint32_t)(g2 * g2);
                m3 += g1 * ss, m4 += g2 * ss;
                M2 += (unsigned long long)(long long)(g1 * g2);
                g[kk][q] = gq;
            }
            M0 += m0, M1 += m1, M3 += (unsigned long long)(long long)m3, M4 += (unsigned long long)(long long)m4;
        }
#else
        // the small instance loads in groups of SRS_LB: a group of four's registers do not fit its budget beside g
        constexpr int LB2 = ONE ? SRS_LB : SR_LB;
#pragma unroll
        for (int kb = 0; kb < KMAX; kb += LB2) {
            if (kb >= K) { // uniform: zeros up to the next multiple of SR_LB (sr_pass reads whole groups)
                if (kb < ((K + SR_LB - 1) & ~(SR_LB - 1)))
#pragma unroll
                    for (int j = 0; j < LB2; j++)
                        if (kb + j < KMAX) sr_dx[(kb + j) * SR_PL + pl] = sr_dx[(KMAX + kb + j) * SR_PL + pl] = 0u;
                continue;
            }
            uint2 xv[LB2];
            int   nin[LB2]; // the chunk's pixels inside the part: 4, fewer in the last column of a crop width that is
                            // not a multiple of 4, none past the part
#pragma unroll
            for (int j = 0; j < LB2; j++) { // the group's loads in flight together
                xv[j] = make_uint2(0u, 0u), nin[j] = 0;
                if (kb + j >= KMAX) continue;
                int row, col;
                chunk_at(kb + j, row, col);
                nin[j]      = pl + (kb + j) * SR_PL < nch ? min(4, uw - 4 * col) : 0;
                const int y = ur.v_start + it.y0 + row, x = ur.h_start + 4 * col;
                xv[j]       = *(const uint2 *)(P.dxp + (size_t)y * P.fstride + x);
                advance();
            }
#pragma unroll
            for (int j = 0; j < LB2; j++) {
                const int kk = kb + j;
                if (kk >= KMAX) break;
                // pixels outside the part read as zeros everywhere: g = 0 and (x - src) = 0 add nothing to any sum
                const uint32_t mlo = nin[j] >= 2 ? ~0u : nin[j] == 1 ? 0xFFFFu : 0u;
                const uint32_t mhi = nin[j] >= 4 ? ~0u : nin[j] == 3 ? 0xFFFFu : 0u;
                g[kk][0] &= mlo, g[kk][2] &= mlo, g[kk][1] &= mhi, g[kk][3] &= mhi;
                const uint2    x2 = make_uint2(xv[j].x & mlo, xv[j].y & mhi);
                const int      dxq[4] = {(int)(int16_t)(x2.x & 0xFFFF), (int)x2.x >> 16, (int)(int16_t)(x2.y & 0xFFFF),
                                         (int)x2.y >> 16};
                const uint32_t fw[4] = {__builtin_amdgcn_perm(g[kk][2], g[kk][0], 0x05040100u),
                                        __builtin_amdgcn_perm(g[kk][2], g[kk][0], 0x07060302u),
                                        __builtin_amdgcn_perm(g[kk][3], g[kk][1], 0x05040100u),
                                        __builtin_amdgcn_perm(g[kk][3], g[kk][1], 0x07060302u)};
                uint32_t m0 = 0, m1 = 0; // <= 4 g^2 < 2^32
                int      m3 = 0, m4 = 0; // |4 g s| < 2^31
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t gq = fw[q] & gmask; // (flt0 - u, flt1 - u); an ep's absent filter reads as 0
                    const int      g1 = (int)(int16_t)(gq & 0xFFFF), g2 = (int)gq >> 16, ss = -(dxq[q] << 4);
                    m0 += (uint32_t)(g1 * g1), m1 += (uint32_t)(g2 * g2);
                    m3 += g1 * ss, m4 += g2 * ss;
                    M2 += (unsigned long long)(long long)(g1 * g2);
                    g[kk][q] = gq;
                }
                M0 += m0, M1 += m1, M3 += (unsigned long long)(long long)m3, M4 += (unsigned long long)(long long)m4;
                sr_dx[kk * SR_PL + pl] = x2.x, sr_dx[(KMAX + kk) * SR_PL + pl] = x2.y;
            }
        }
#endif
        {
            const unsigned long long t[5] = {wave_sum_u64_limbs(M0), wave_sum_u64_limbs(M1), wave_sum_u64_limbs(M2),
                                             wave_sum_u64_limbs(M3), wave_sum_u64_limbs(M4)};
            if ((pl & 63) == WAVE_LAST)
#pragma unroll
                for (int q = 0; q < 5; q++) s_red[pl >> 6][q] = t[q];
        }
        __syncthreads(); // B1: the moments are in s_red
        __syncthreads(); // B2: the first tree is in s_xq
        // diagnostics (stat): pixel wave 0's pass time (B2/B4 release to its arrival at B3) and its wait from B3 to the
        // B4 release
        unsigned long long tpass = 0, twait = 0, tmark = stat ? __builtin_amdgcn_s_memrealtime() : 0;
        if (ONE || (!TREE && it.nparts == 1 && !(xmode & 0x200))) {
            // One barrier per pass, and no wave waits on another's descent step: every wave (pixel and control) holds
            // the seeded descent in its own scalar registers and steps it itself from the pass's wave partials --
            // report + next once per pass, the same decisions everywhere (the errors are the same LDS words).  Before
            // this the control wave stepped the descent and built both children of every candidate (three steps per
            // pass, serial) while the pixel waves waited at the barrier: 13 us of descent per item, 8 of them control
            Descent  Dw   = uniform(s_desc);
            bool     live = __builtin_amdgcn_readfirstlane(s_nv) != 0;
            uint32_t xq   = 0;
            {
                int32_t x[2];
                decode_xq(Dw, x);
                xq = __builtin_amdgcn_readfirstlane(pack2(x[0], x[1]));
            }
            for (int pass = 1; live; pass++) {
                const uint32_t xl[1] = {xq};
                sr_pass<1>(g, sr_dx, pl, K, 1, xl, s_red2[pass & 1]);
                if (stat) {
                    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                    tpass += t - tmark, tmark = t;
                }
                __syncthreads(); // B3: the pass's wave partials are in LDS
                unsigned long long e0 = 0;
#pragma unroll
                for (int w = 0; w < SR_PW; w++) e0 += s_red2[pass & 1][w][0];
                Dw.report(readlane64((long long)e0, 0));
                live = Dw.next() && pass <= SR_MAX_PASSES;
                if (live) {
                    int32_t x[2];
                    decode_xq(Dw, x);
                    xq = __builtin_amdgcn_readfirstlane(pack2(x[0], x[1]));
                }
                if (stat) {
                    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                    twait += t - tmark, tmark = t;
                }
            }
        } else if (!TREE && !(xmode & 0x200)) {
            // Row parts, self-stepping: the control wave sums this part's wave partials, exchanges the sum with the
            // other parts and leaves the frame-unit total in LDS (B4); then every wave steps its own copy of the
            // descent -- no children built, no wave waits on another's step
            Descent  Dw   = uniform(s_desc);
            bool     live = __builtin_amdgcn_readfirstlane(s_nv) != 0;
            uint32_t xq   = 0;
            {
                int32_t x[2];
                decode_xq(Dw, x);
                xq = __builtin_amdgcn_readfirstlane(pack2(x[0], x[1]));
            }
            for (int pass = 1; live; pass++) {
                const uint32_t xl[1] = {xq};
                sr_pass<1>(g, sr_dx, pl, K, 1, xl, s_red);
                if (stat) {
                    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                    tpass += t - tmark, tmark = t;
                }
                __syncthreads(); // B3: the pass's wave partials are in s_red
                __syncthreads(); // B4: the parts' total is in s_etot
                const bool okx = __builtin_amdgcn_readfirstlane(s_xok[pass & 1]) != 0;
                if (okx) {
                    Dw.report(readlane64((long long)s_etot[pass & 1], 0));
                    live = Dw.next() && pass <= SR_MAX_PASSES;
                } else
                    live = false;
                if (live) {
                    int32_t x[2];
                    decode_xq(Dw, x);
                    xq = __builtin_amdgcn_readfirstlane(pack2(x[0], x[1]));
                }
                if (stat) {
                    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                    twait += t - tmark, tmark = t;
                }
            }
        } else
        for (;;) {
            const int nv = __builtin_amdgcn_readfirstlane(s_nv);
            if (nv == 0) break;
            if constexpr (!TREE) {
                sr_pass<1>(g, sr_dx, pl, K, 1, s_xq, s_red);
            } else {
                switch (nv) {
                case 1: sr_pass<1>(g, sr_dx, pl, K, nv, s_xq, s_red); break;
                case 2: sr_pass<2>(g, sr_dx, pl, K, nv, s_xq, s_red); break;
                case 3: sr_pass<3>(g, sr_dx, pl, K, nv, s_xq, s_red); break;
                case 4: sr_pass<4>(g, sr_dx, pl, K, nv, s_xq, s_red); break;
                default: sr_pass<SG_NC>(g, sr_dx, pl, K, nv, s_xq, s_red); break;
                }
            }
            if (stat) {
                const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                tpass += t - tmark, tmark = t;
            }
            __syncthreads(); // B3: the pass's errors are in s_red
            __syncthreads(); // B4: the next tree (or the end) is in s_xq / s_nv
            if (stat) {
                const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                twait += t - tmark, tmark = t;
            }
        }
        if (stat && pl == 0) atomicAdd(stat + 7, tpass), atomicAdd(stat + 8, twait);
    } else {
        // ================= control wave =================
        // stat (SVTGPU_SR_STATS diagnostics, else null): items, passes, candidate-pixels, load / descent / control
        // ticks (100 MHz), pixels.  The control steps are the item's serial critical path: this wave issues ahead of
        // the other workgroup's pixel waves on its SIMD (it waits at the barriers otherwise)
        __builtin_amdgcn_s_setprio(3);
        const int                lane = threadIdx.x & 63;
        const unsigned long long t0   = stat ? __builtin_amdgcn_s_memrealtime() : 0;
        unsigned long long       tctl = 0, ncp = 0, tpre = 0;
        __syncthreads(); // B1
        const unsigned long long t1 = stat ? __builtin_amdgcn_s_memrealtime() : 0;
        long long v  = 0; // lane q < 5: moment q over the workgroup (and the other row parts)
        bool      ok = true;
        if (lane < 5) {
            unsigned long long t = 0;
            for (int w = 0; w < SR_PW; w++) t += s_red[w][lane];
            v = (long long)t;
            if (!ONE && it.nparts > 1) ok = sr_exchange_lane(xch, it, 0, lane, v, status, xmode);
        }
        ok = __ballot(!ok) == 0;
        long long mv[5];
#pragma unroll
        for (int q = 0; q < 5; q++) mv[q] = readlane64(v, q);
        // the descent is wave-uniform from here on: kept in scalar registers, stepped by the scalar unit
        Descent D = uniform(sgr_seed(A, p, it.pair, (const int64_t *)mv, cfg));
        D.next(); // the seed itself is the first candidate
        sr_tree_publish(D, ok, nodes, s_xq, &s_mask, &s_nv);
        if (ONE || (!TREE && it.nparts == 1 && !(xmode & 0x200))) {
            // the self-stepping path (see the pixel waves): the seeded descent to LDS for every wave, then the same
            // report + next per pass as everyone else
            if (lane == 0) s_desc = D;
            __syncthreads(); // B2
            bool live = ok;
            int  pass = 1;
            for (; live; pass++) {
                __syncthreads(); // B3
                const unsigned long long tb = stat ? __builtin_amdgcn_s_memrealtime() : 0;
                ncp += (unsigned long long)nch * 4;
                unsigned long long e0 = 0;
#pragma unroll
                for (int w = 0; w < SR_PW; w++) e0 += s_red2[pass & 1][w][0];
                D.report(readlane64((long long)e0, 0));
                live = D.next() && pass <= SR_MAX_PASSES;
                if (pass > SR_MAX_PASSES && lane == 0) atomicOr(status, 1);
                if (stat) tctl += __builtin_amdgcn_s_memrealtime() - tb;
            }
            if (stat && lane == 0) atomicAdd(stat + 1, (unsigned long long)(pass - 1));
        } else if (!TREE && nodes == 1 && !(xmode & 0x200)) {
            // self-stepping row parts (see the pixel waves): the exchange between B3 and B4, the step after B4
            if (lane == 0) s_desc = D;
            __syncthreads(); // B2
            bool live = ok;
            int  pass = 1;
            for (; live; pass++) {
                __syncthreads(); // B3
                const unsigned long long tb = stat ? __builtin_amdgcn_s_memrealtime() : 0;
                ncp += (unsigned long long)nch * 4;
                if (lane == 0) {
                    unsigned long long t = 0;
                    for (int w = 0; w < SR_PW; w++) t += s_red[w][0];
                    long long e   = (long long)t;
                    const bool ex = sr_exchange_lane(xch, it, pass, 0, e, status, xmode);
                    s_etot[pass & 1] = (unsigned long long)e, s_xok[pass & 1] = ex;
                }
                __syncthreads(); // B4
                const bool okx = __builtin_amdgcn_readfirstlane(s_xok[pass & 1]) != 0;
                if (okx) {
                    D.report(readlane64((long long)s_etot[pass & 1], 0));
                    live = D.next() && pass <= SR_MAX_PASSES;
                    if (pass > SR_MAX_PASSES && lane == 0) atomicOr(status, 1);
                } else
                    live = false;
                if (stat) tctl += __builtin_amdgcn_s_memrealtime() - tb;
            }
            if (stat && lane == 0) atomicAdd(stat + 1, (unsigned long long)(pass - 1));
        } else {
        __syncthreads(); // B2
        for (int pass = 1;; pass++) {
            const int nv = __builtin_amdgcn_readfirstlane(s_nv);
            if (nv == 0) break;
            const uint32_t mask = __builtin_amdgcn_readfirstlane(s_mask);
            uint32_t       xw = 0, xb = 0;
            bool           okw = false, okb = false;
            const unsigned long long tc0 = stat ? __builtin_amdgcn_s_memrealtime() : 0;
            if (nodes == 1) sr_children(D, xw, okw, xb, okb); // during the pass
            if (stat) tpre += __builtin_amdgcn_s_memrealtime() - tc0;
            __syncthreads(); // B3
            const unsigned long long tb = stat ? __builtin_amdgcn_s_memrealtime() : 0;
            ncp += (unsigned long long)nv * nch * 4;
            long long e = 0; // lane c < nv: compacted candidate c's error
            ok = true;
            if (lane < nv) {
                unsigned long long t = 0;
                for (int w = 0; w < SR_PW; w++) t += s_red[w][lane];
                e = (long long)t;
                if (!ONE && it.nparts > 1) ok = sr_exchange_lane(xch, it, pass, lane, e, status, xmode);
            }
            ok = __ballot(!ok) == 0;
            if (pass > SR_MAX_PASSES) {
                if (lane == 0) atomicOr(status, 1);
                ok = false;
            }
            if (nodes == 1) { // the outcome picks a prepared child; the descent itself steps after the barrier
                const long long e0    = readlane64(e, 0);
                const bool      worse = !D.init && e0 > D.err;
                if (lane == 0) {
                    s_xq[0] = worse ? xw : xb;
                    s_mask  = 1;
                    s_nv    = ok && (worse ? okw : okb) ? 1 : 0;
                }
                if (stat) tctl += __builtin_amdgcn_s_memrealtime() - tb;
                __syncthreads(); // B4
                if (stat && lane == 0 && s_nv == 0) atomicAdd(stat + 1, (unsigned long long)pass);
                if (ok) { // the same state change as the choice above, with the error value kept
                    D.report(e0);
                    D.next();
                }
                continue;
            }
            if (ok) { // the same steps in every lane (the errors made uniform: scalar code)
                long long ev[SG_NC];
#pragma unroll
                for (int c = 0; c < SG_NC; c++) ev[c] = c < nv ? readlane64(e, c) : 0;
                sgr_replay(D, mask, [&](int node) {
                    const int i = __popc(mask & ((1u << node) - 1));
                    long long r = ev[0];
#pragma unroll
                    for (int c = 1; c < SG_NC; c++) r = i == c ? ev[c] : r;
                    return (int64_t)r;
                });
            }
            sr_tree_publish(D, ok && !D.done, nodes, s_xq, &s_mask, &s_nv);
            if (stat) tctl += __builtin_amdgcn_s_memrealtime() - tb;
            __syncthreads(); // B4
            if (stat && lane == 0 && s_nv == 0) atomicAdd(stat + 1, (unsigned long long)pass);
        }
        }
        if (lane == 0 && it.part == 0) ds[it.pair] = D;
        if (stat && lane == 0) {
            const unsigned long long te = __builtin_amdgcn_s_memrealtime();
            atomicAdd(stat + 0, 1ull), atomicAdd(stat + 2, ncp), atomicAdd(stat + 3, t1 - t0);
            atomicAdd(stat + 4, te - t1), atomicAdd(stat + 5, tctl);
            atomicAdd(stat + 6, (unsigned long long)nch * 4), atomicAdd(stat + 9, tpre);
            if (it.nparts > 1) // the row-part items apart: count, load, descent, control ticks
                atomicAdd(stat + 10, 1ull), atomicAdd(stat + 11, t1 - t0), atomicAdd(stat + 12, te - t1),
                    atomicAdd(stat + 13, tctl);
            if (it.nparts == 1 && K <= SRS_KMAX) // the items of the small instance's size apart, wherever they run
                atomicAdd(stat + 16, 1ull), atomicAdd(stat + 17, t1 - t0), atomicAdd(stat + 18, te - t1),
                    atomicAdd(stat + 19, tctl);
        }
    }
    PROF_END(tk);
