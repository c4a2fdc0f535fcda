// cdef_pick_plan_check — the integer rules of the frame-level CDEF strength pick (csrc/cdef_pick_plan.h) against the CPU
// oracle (oracle/cdef_oracle.c), checked without a GPU: the greedy schedule against the reference's joint search, the
// launch path replayed on the host (the lists and values the step kernels leave) with the settle check applied at every
// checkpoint, the RD choice / per-FB assignment / parameter conversion against oracle_cdef_pick, the buffer layouts,
// the checkpoint policy and the environment switches.  Built and run by tests/test_cdef_pick_plan.py; prints every
// violated check, exit status 1 if any.
#include <cstdio>
#include <string>
#include <vector>

#include "../oracle/oracle.h"
#include "../svt-av1_pro-anchor-v2.1.0-_amd/csrc/cdef_pick_plan.h"

static int         g_fail = 0;
static std::string g_case;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++g_fail <= 40) {                                             \
                std::fprintf(stderr, "%s: %s: ", g_case.c_str(), #cond);      \
                std::fprintf(stderr, __VA_ARGS__);                            \
                std::fprintf(stderr, "\n");                                   \
            }                                                                 \
        }                                                                     \
    } while (0)

static uint32_t g_rng = 1;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

// ---- the schedule against the reference's joint search (joint_search_ in oracle/cdef_oracle.c, EbEncCdef.c:697-727) ----
struct Call {
    int nb_sel, shifted; // the selection size of a call of svt_search_one_dual; a shift of the list precedes it
};
static std::vector<Call> reference_calls(int nb) {
    std::vector<Call> v;
    for (int i = 0; i < nb; i++) v.push_back({i, 0});
    for (int i = 0; i < 4 * nb; i++) v.push_back({nb - 1, 1});
    return v;
}
static long check_schedule() {
    long total = 0;
    for (int c = 0; c < PICK_MAX_CHAINS; c++) {
        g_case = "schedule of chain " + std::to_string(c);
        const int               nb = 1 << c;
        const std::vector<Call> want = reference_calls(nb);
        CHECK(pick_chain_nb(c) == nb && pick_chain_calls(c) == 5 * nb && (int)want.size() == 5 * nb, "5 nb calls");
        std::vector<Call> got;
        int               finish = -1;
        for (int step = 0; step <= PICK_NSTEPS; step++) {
            const PickChainStep C = pick_chain_step(c, step);
            CHECK(C.nb == nb, "step %d: nb %d", step, C.nb);
            if (C.nb_sel >= 0) {
                got.push_back({C.nb_sel, C.shift});
                CHECK(finish < 0, "step %d: a call after the finishing step", step);
            } else if (C.nb_sel == PICK_FINISH) {
                CHECK(finish < 0, "step %d: a second finishing step", step);
                finish = step;
                CHECK(!C.shift, "the finishing step shifts");
            } else {
                CHECK(C.nb_sel == PICK_ENDED && finish >= 0 && step > finish, "step %d: nb_sel %d", step, C.nb_sel);
                CHECK(C.prev == -1 && !C.shift, "step %d: an ended chain folds a result (prev %d, shift %d)", step, C.prev, C.shift);
            }
            // the result folded in at this step is the previous call's: slot = that call's selection size
            if (C.nb_sel != PICK_ENDED) {
                const int prev = step == 0 ? -1 : pick_chain_step(c, step - 1).nb_sel;
                CHECK(C.prev == prev, "step %d: prev %d, the previous call's size %d", step, C.prev, prev);
            }
        }
        CHECK(finish == 5 * nb, "finishing step %d", finish);
        CHECK(got.size() == want.size(), "%zu calls, the reference makes %zu", got.size(), want.size());
        for (size_t i = 0; i < got.size() && i < want.size(); i++)
            CHECK(got[i].nb_sel == want[i].nb_sel && got[i].shifted == want[i].shifted, "call %zu: size %d shift %d, the reference %d %d",
                  i, got[i].nb_sel, got[i].shifted, want[i].nb_sel, want[i].shifted);
        total += (long)got.size();
    }
    g_case = "schedule";
    CHECK(total == 75, "%ld calls in all", total);
    return total;
}

// ---- tables ----
struct Table {
    std::string           name;
    int                   nfb, level; // blocks of the frame (a row of 64x64 blocks); the controls' level
    std::vector<uint64_t> mse;        // [2][nfb][64]
    std::vector<uint8_t>  skip;       // [nfb]
    int                   live() const {
        int n = 0;
        for (uint8_t s : skip) n += !s;
        return n;
    }
};
// convex per-FB strength curves with a random optimum and scale per FB, as tests/test_cdef_gpu.py's settled-chains
// tables; every third block of the frame's tail skipped
static Table convex_table(uint32_t seed, int nfb, int level, int scale_bits) {
    Table t;
    t.name = "convex seed " + std::to_string(seed) + ", " + std::to_string(nfb) + " blocks, level " + std::to_string(level);
    t.nfb = nfb, t.level = level;
    t.mse.resize((size_t)2 * nfb * 64);
    t.skip.assign(nfb, 0);
    g_rng = seed * 2654435761u + 12345u;
    for (int p = 0; p < 2; p++)
        for (int fb = 0; fb < nfb; fb++) {
            const int      opt   = (int)(rnd() >> 26);
            const uint64_t scale = (1u << 10) + (rnd() >> (32 - scale_bits));
            for (int j = 0; j < 64; j++) t.mse[((size_t)p * nfb + fb) * 64 + j] = scale * (uint64_t)(64 + (j - opt) * (j - opt)) + (rnd() >> 20);
        }
    for (int fb = nfb - 4; fb < nfb; fb += 3) t.skip[fb] = 1;
    return t;
}
static Table const_table(int nfb, int level) {
    Table t;
    t.name = "all entries equal, " + std::to_string(nfb) + " blocks, level " + std::to_string(level);
    t.nfb = nfb, t.level = level;
    t.mse.assign((size_t)2 * nfb * 64, 123457);
    t.skip.assign(nfb, 0);
    t.skip[1] = 1;
    return t;
}
// Seeds chosen on the CPU, by this program's counts over seeds 0 .. 1499, so that settled and unsettled chains both
// occur.  Tables this small nearly always settle (chain 0 always does: its state is empty): seeds 0 .. 8 and the
// all-tie tables give settled chains of every length at 4, 16 and 64 strengths; seeds 56, 899, 1064 and 1262 (all 64
// strengths) each leave one chain unsettled through its last call: chains 1, 2, 3 and 1.
static std::vector<Table> tables() {
    std::vector<Table> v;
    const int levels[3] = {12, 5, 1}; // 4, 16 and 64 strengths
    for (int l = 0; l < 3; l++) v.push_back(const_table(10 + 9 * l, levels[l]));
    for (uint32_t seed : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 56u, 899u, 1064u, 1262u})
        v.push_back(convex_table(seed, 10 + (int)(seed * 7 % 33), levels[seed % 3], seed & 1 ? 20 : 14));
    return v;
}

// ---- the launch path replayed on the host ----
struct Compact {
    int                     n = 0, end = 0;
    std::vector<uint64_t>   wmse;    // [n][2][64] bias applied (pick_gather_kernel)
    std::vector<int>        fb_of;   // row -> FB
    std::vector<uint64_t *> row[2];  // the oracle's view
};
static void compact(const Table &t, const SvtGpuCdefControls &ctrls, Compact &C) {
    C.end = ctrls.first_pass_fs_num + ctrls.default_second_pass_fs_num;
    for (int fb = 0; fb < t.nfb; fb++)
        if (!t.skip[fb]) C.fb_of.push_back(fb);
    C.n = (int)C.fb_of.size();
    C.wmse.resize((size_t)C.n * 128);
    for (int i = 0; i < C.n; i++)
        for (int p = 0; p < 2; p++)
            for (int g = 0; g < 64; g++) {
                uint64_t v = t.mse[((size_t)p * t.nfb + C.fb_of[i]) * 64 + g];
                if (ctrls.zero_fs_cost_bias && g == 0) v = ((uint64_t)ctrls.zero_fs_cost_bias * v) >> 6;
                C.wmse[((size_t)i * 2 + p) * 64 + g] = v;
            }
    for (int p = 0; p < 2; p++) {
        C.row[p].resize(C.n + 1);
        for (int i = 0; i < C.n; i++) C.row[p][i] = &C.wmse[((size_t)i * 2 + p) * 64];
    }
}
struct Replay {
    int32_t  lev[(PICK_NSTEPS + 1) * PICK_MAX_CHAINS * 32];
    uint64_t val[(PICK_NSTEPS + 1) * PICK_MAX_CHAINS];
    int32_t  fin[PICK_MAX_CHAINS * 32];
    uint64_t best[PICK_MAX_CHAINS];
};
constexpr int32_t  POISON   = 0x7f7f7f7f;
constexpr uint64_t POISON64 = 0x7f7f7f7f7f7f7f7full;
// what sod_step_kernel's launches 0 .. NSTEPS leave: lev[s] the selection entering call s, val[s] the value of call
// s - 1, fin / best at each chain's finishing step; every call made by oracle_search_one_dual
static void replay(Compact &C, Replay &R) {
    for (auto &x : R.lev) x = POISON;
    for (auto &x : R.val) x = POISON64;
    for (auto &x : R.fin) x = POISON;
    for (auto &x : R.best) x = POISON64;
    uint64_t **mse[2] = {C.row[0].data(), C.row[1].data()};
    for (int c = 0; c < PICK_MAX_CHAINS; c++) {
        int      res0 = 0, res1 = 0;
        uint64_t resv = 0;
        for (int step = 0; step <= PICK_NSTEPS; step++) {
            const PickChainStep S = pick_chain_step(c, step);
            if (S.nb_sel == PICK_ENDED) continue;
            int32_t sl[32];
            for (int i = 0; i < 32; i++) sl[i] = step ? R.lev[pick_lev_at(step - 1, c, i)] : 0;
            if (S.prev >= 0) {
                sl[S.prev] = res0, sl[16 + S.prev] = res1;
                if (S.shift)
                    for (int q = 0; q < S.nb - 1; q++) sl[q] = sl[q + 1], sl[16 + q] = sl[16 + q + 1];
                R.val[pick_val_at(step, c)] = resv;
                if (S.nb_sel == PICK_FINISH) R.best[c] = resv;
            }
            if (S.nb_sel == PICK_FINISH) {
                for (int i = 0; i < 32; i++) R.fin[c * 32 + i] = sl[i];
                continue;
            }
            for (int i = 0; i < 32; i++) R.lev[pick_lev_at(step, c, i)] = sl[i];
            int lev0[17], lev1[17];
            for (int i = 0; i < 16; i++) lev0[i] = sl[i], lev1[i] = sl[16 + i];
            resv = oracle_search_one_dual(lev0, lev1, S.nb_sel, mse, C.n, 0, C.end);
            res0 = lev0[S.nb_sel], res1 = lev1[S.nb_sel];
        }
    }
}
// the reference's joint search of nb strengths, transcribed (joint_search_ is static in the oracle)
static uint64_t joint_search(int *lev0, int *lev1, int nb, Compact &C) {
    uint64_t **mse[2] = {C.row[0].data(), C.row[1].data()};
    uint64_t   r      = (uint64_t)1 << 63;
    for (int i = 0; i < nb; i++) r = oracle_search_one_dual(lev0, lev1, i, mse, C.n, 0, C.end);
    for (int i = 0; i < 4 * nb; i++) {
        for (int j = 0; j < nb - 1; j++) lev0[j] = lev0[j + 1], lev1[j] = lev1[j + 1];
        r = oracle_search_one_dual(lev0, lev1, nb - 1, mse, C.n, 0, C.end);
    }
    return r;
}

static long g_settled = 0, g_unsettled = 0, g_copies = 0;

static void check_replay_and_settle(Compact &C, const Replay &R) {
    const std::string name = g_case;
    for (int c = 0; c < PICK_MAX_CHAINS; c++) {
        const int nb = 1 << c, L = 5 * nb;
        g_case = name + ", chain " + std::to_string(c);
        int lev0[17] = {0}, lev1[17] = {0};
        const uint64_t want = joint_search(lev0, lev1, nb, C);
        CHECK(R.best[c] == want, "value %llu, the joint search %llu", (unsigned long long)R.best[c], (unsigned long long)want);
        for (int i = 0; i < 16; i++)
            CHECK(R.fin[c * 32 + i] == (i < nb ? lev0[i] : 0) && R.fin[c * 32 + 16 + i] == (i < nb ? lev1[i] : 0), "final list entry %d: %d / %d", i,
                  R.fin[c * 32 + i], R.fin[c * 32 + 16 + i]);
        const int at_full = pick_settle_chain(R.lev, c, PICK_NSTEPS).at; // every step seen
        CHECK(at_full >= 2 * nb && at_full <= L, "at %d", at_full);
        (at_full < L ? g_settled : g_unsettled)++;
        for (int T = 16; T < PICK_NSTEPS; T++) {
            // the check sees what steps 0 .. T wrote
            Replay V = R;
            for (int s = T + 1; s <= PICK_NSTEPS; s++) {
                for (int i = 0; i < 32; i++) V.lev[pick_lev_at(s, c, i)] = POISON;
                V.val[pick_val_at(s, c)] = POISON64;
            }
            const PickSettle S = pick_settle_chain(V.lev, c, T);
            CHECK(S.at == (at_full <= T ? at_full : L), "T %d: at %d, over the whole run %d", T, S.at, at_full);
            CHECK(S.finished == (L <= T) && S.settled == (S.finished || S.at <= T), "T %d: finished %d settled %d", T, S.finished, S.settled);
            CHECK(S.copies() == (S.settled && !S.finished), "T %d: copies", T);
            if (!S.copies()) continue;
            g_copies++;
            CHECK(S.a >= nb && S.a < T && S.b >= nb && S.b <= T, "T %d: a %d b %d", T, S.a, S.b);
            int32_t  fin[PICK_MAX_CHAINS * 32];
            uint64_t best[PICK_MAX_CHAINS];
            for (auto &x : fin) x = POISON;
            for (auto &x : best) x = POISON64;
            pick_settle_write(V.lev, V.val, c, S, fin, best);
            CHECK(best[c] == R.best[c], "T %d: value %llu from step %d, the chain run to its end %llu", T, (unsigned long long)best[c], S.a + 1,
                  (unsigned long long)R.best[c]);
            for (int i = 0; i < 32; i++) CHECK(fin[c * 32 + i] == R.fin[c * 32 + i], "T %d: final list entry %d: %d, run to its end %d", T, i, fin[c * 32 + i], R.fin[c * 32 + i]);
            for (int o = 0; o < PICK_MAX_CHAINS; o++)
                if (o != c) CHECK(fin[o * 32] == POISON && best[o] == POISON64, "T %d: chain %d's result written", T, o);
        }
    }
    g_case = name;
}

// ---- the RD choice, the per-FB assignment and the parameters against oracle_cdef_pick ----
static long check_end_to_end(const Table &t, const SvtGpuCdefControls &ctrls, Compact &C, const Replay &R) {
    const std::string name = g_case;
    const uint64_t    lambdas[] = {0, 1, 60000, (uint64_t)1 << 30};
    long              n = 0;
    for (uint64_t lambda : lambdas)
        for (int q : {0, 128, 255}) {
            g_case = name + ", lambda " + std::to_string(lambda) + ", q " + std::to_string(q);
            SvtGpuCdefParams    want;
            std::vector<int8_t> want_fbs(t.nfb, 99), got_fbs(t.nfb, 0);
            CHECK(oracle_cdef_pick(64 * t.nfb, 64, t.mse.data(), t.skip.data(), &ctrls, q, lambda, &want, want_fbs.data()) == SVTGPU_OK, "oracle_cdef_pick");
            const PickChoice ch = pick_rd_choice(R.best, C.n, lambda);
            CHECK(ch.nbits >= 0 && ch.nbits < PICK_MAX_CHAINS && (ch.chain == ch.nbits || ch.chain == -1), "choice %d / %d", ch.nbits, ch.chain);
            int32_t gi[32];
            pick_chosen_list(R.fin, ch, gi);
            for (int i = 0; i < C.n; i++) got_fbs[C.fb_of[i]] = (int8_t)pick_fb_strength(C.row[0][i], C.row[1][i], gi, 1 << ch.nbits);
            const SvtGpuCdefParams got = pick_params_from(pick_map_from(ctrls, q), ch.nbits, gi);
            CHECK(!std::memcmp(&got, &want, sizeof want), "parameters: bits %d damping %d y0 %d uv0 %d, the oracle %d %d %d %d", got.cdef_bits,
                  got.cdef_damping, got.cdef_y_strength[0], got.cdef_uv_strength[0], want.cdef_bits, want.cdef_damping, want.cdef_y_strength[0],
                  want.cdef_uv_strength[0]);
            CHECK(got_fbs == want_fbs, "per-FB strengths");
            n++;
        }
    g_case = name;
    return n;
}

static long check_tables() {
    long n = 0;
    for (const Table &t : tables()) {
        g_case = t.name;
        SvtGpuCdefControls ctrls;
        CHECK(oracle_cdef_controls_for_level(t.level, &ctrls) == SVTGPU_OK, "controls");
        Compact C;
        compact(t, ctrls, C);
        CHECK(C.n >= 8 && C.n <= 40 && (C.end == 4 || C.end == 16 || C.end == 64), "%d live blocks, %d strengths", C.n, C.end);
        Replay R;
        replay(C, R);
        check_replay_and_settle(C, R);
        n += check_end_to_end(t, ctrls, C, R);
    }
    g_case = "tables";
    CHECK(g_settled > 0 && g_unsettled > 0 && g_copies > 0, "%ld settled and %ld unsettled (chain, table) pairs, %ld checks that copy", g_settled,
          g_unsettled, g_copies);
    return n;
}

// ---- the layouts ----
struct Region {
    const char *name;
    size_t      off, bytes;
};
static void check_regions(const char *buf, size_t alloc, const std::vector<Region> &r) {
    for (size_t i = 0; i < r.size(); i++) {
        CHECK(r[i].off + r[i].bytes <= alloc, "%s: %s ends at %zu of %zu bytes", buf, r[i].name, r[i].off + r[i].bytes, alloc);
        for (size_t j = 0; j < i; j++)
            CHECK(r[i].off >= r[j].off + r[j].bytes || r[j].off >= r[i].off + r[i].bytes, "%s: %s overlaps %s", buf, r[i].name, r[j].name);
    }
}
static long check_layout() {
    const size_t sizes[] = {1, 2, 3, 5, 65, 510, 2040, 2304, 8160};
    for (size_t nfb : sizes) {
        g_case = "layout of " + std::to_string(nfb) + " blocks";
        const PickLayout L(nfb);
        const size_t     nlev = (size_t)(PICK_NSTEPS + 1) * PICK_MAX_CHAINS;
        check_regions("d_pick_part", L.part_words * 8,
                      {{"wmse", L.part_wmse * 8, nfb * 128 * 8}, {"tot", L.part_tot * 8, (size_t)3 * 4 * 4096 * 8}, {"val", L.part_val * 8, nlev * 8},
                       {"wmse32", L.part_wmse32 * 8, nfb * 128 * 4}});
        CHECK(L.part_words == nfb * 128 + (size_t)3 * 4 * 4096 + 41 * 4 + nfb * 64, "d_pick_part: %zu words", L.part_words);
        CHECK(L.part_wmse32 * 8 % 16 == 0, "wmse32 at byte %zu", L.part_wmse32 * 8);
        check_regions("d_pick_lev", L.lev_words * 4, {{"lev", L.lev_lev * 4, nlev * 32 * 4}, {"fin", L.lev_fin * 4, 4 * 32 * 4}, {"wide", L.lev_wide * 4, 4}});
        CHECK(L.lev_wide == L.lev_fin + 161 && L.lev_fin == 41 * 4 * 32 && L.lev_words == 41 * 4 * 32 + 4 * 32 + 64, "d_pick_lev: fin %zu wide %zu of %zu",
              L.lev_fin, L.lev_wide, L.lev_words);
        CHECK(L.out_words * 8 >= PICK_MAX_CHAINS * sizeof(uint64_t) && L.out_words == 8, "d_pick_out");
        check_regions("d_fb_list", L.list_words * 4, {{"list", L.list_fb * 4, nfb * 4}, {"count", L.list_count * 4, 4}, {"inv", L.list_inv * 4, nfb * 4}});
        CHECK(L.list_words == 2 * nfb + 1, "d_fb_list: %zu words", L.list_words);
        check_regions("d_pick_xch", L.xch_bytes,
                      {{"part", L.xch_part * 8, (size_t)PS_NCH * 4 * 4096 * 8}, {"amin", L.xch_amin * 8, 4 * 64 * 2 * 8}, {"status", L.xch_status * 8, 4},
                       {"stat", L.xch_stat * 8, 4 * 8}});
        CHECK(L.xch_status == L.xch_amin + 4 * 64 * 2 && L.xch_stat == L.xch_status + 8, "status and diagnostics at +0 and +8 words after the row minima");
        CHECK(L.xch_bytes == (size_t)(64 * 4 * 4096 + 4 * 64 * 2 + 16) * 8 && SVTGPU_PICK_XCH_BYTES == L.xch_bytes, "d_pick_xch: %zu bytes", L.xch_bytes);
        check_regions("d_apick", L.apick_bytes, {{"flag", L.apick_flag, 4}, {"dep", L.apick_dep, 4}, {"params", L.apick_params, sizeof(SvtGpuCdefParams)}});
        CHECK(L.apick_flag == 0 && L.apick_dep == 8 && L.apick_params == 16 && L.apick_bytes == 64, "d_apick");
        check_regions("h_pick", L.rec_bytes, {{"PickOut", L.rec_out, sizeof(PickOut)}, {"SettleOut", L.rec_settle, sizeof(SettleOut)}, {"strengths", L.rec_fbs, nfb}});
        CHECK(L.rec_out == 0 && L.rec_settle == 448 && L.rec_fbs == 512 && L.rec_bytes == 512 + nfb, "h_pick");
        CHECK(L.rec_out % 8 == 0 && offsetof(PickOut, best) % 8 == 0 && L.rec_settle % 8 == 0, "64-bit alignment of the records");
    }
    // shapes: the persistent kernel's chunks hold the frame exactly while ps_fits; a step's chunk stays in its bounds
    g_case = "launch shapes";
    PickKnobs K{};
    pick_knobs_read_process(K);
    for (int nfb = 1; nfb <= 8160; nfb++) {
        if (ps_fits(nfb)) CHECK(ps_chunk(nfb) >= 1 && ps_chunk(nfb) <= PS_CH && ps_chunk(nfb) * PS_NCH >= nfb, "%d blocks: persistent chunk %d", nfb, ps_chunk(nfb));
        for (int na = 1; na <= PICK_MAX_CHAINS; na++) {
            const PickStepShape sh = pick_step_shape(K, nfb, na);
            CHECK(sh.chunk >= 4 && sh.chunk <= PICK_CHUNK && sh.parts * sh.chunk >= nfb && (sh.parts - 1) * sh.chunk < nfb && sh.grid == 4 * sh.parts * na &&
                      sh.lds == (size_t)sh.chunk * (PICK_MROW * 4 + 8),
                  "%d blocks, %d chains: chunk %d parts %d", nfb, na, sh.chunk, sh.parts);
        }
    }
    CHECK(ps_fits(2048) && !ps_fits(2049), "the persistent kernel's capacity");
    return (long)(sizeof sizes / sizeof sizes[0]);
}

// ---- the checkpoint policy ----
static long check_policy() {
    long n = 0;
    g_case = "policy";
    {
        PickSettlePolicy P;
        CHECK(P.begin(true) == 24, "the first pick checks after step 24");
    }
    // random outcome sequences, both callers: T stays in [16, NSTEPS], a settled outcome at k gives max(k, 16) next
    for (int async_ = 0; async_ <= 1; async_++)
        for (uint32_t seed = 1; seed <= 50; seed++) {
            g_rng = seed;
            PickSettlePolicy P;
            bool             have = false, settled = false; // asynchronous: the record the next pick takes
            int              step = 0;
            for (int pick = 0; pick < 200; pick++, n++) {
                int expect = -1; // asynchronous: the record of the previous pick's check is taken at the start of this one
                if (async_ && have) {
                    P.outcome_async(settled, step), have = false;
                    if (settled) expect = std::max(step, 16);
                }
                const int T = P.begin(true);
                CHECK(T >= 16 && T <= PICK_NSTEPS, "T %d", T);
                if (expect >= 0) CHECK(T == expect, "T %d after a settled outcome at %d", T, step);
                if (T == PICK_NSTEPS) continue; // no check
                CHECK(T <= PICK_NSTEPS - 4, "a check at %d", T);
                settled = rnd() >> 31, step = settled ? (int)(rnd() % (uint32_t)(T + 1)) : PICK_NSTEPS;
                if (async_) have = true;
                else {
                    P.outcome_sync(settled, step, T);
                    if (settled) {
                        PickSettlePolicy Q = P;
                        CHECK(Q.begin(true) == std::max(step, 16), "T %d after a settled outcome at %d", Q.begin(true), step);
                    }
                }
            }
        }
    // two consecutive misses: exactly 8 picks without a check, then a check at 24
    for (int async_ = 0; async_ <= 1; async_++) {
        PickSettlePolicy P;
        int              T = P.begin(true);
        async_ ? P.outcome_async(false, PICK_NSTEPS) : P.outcome_sync(false, PICK_NSTEPS, T);
        T = P.begin(true);
        CHECK(T == 28, "the check after one miss at %d", T);
        async_ ? P.outcome_async(false, PICK_NSTEPS) : P.outcome_sync(false, PICK_NSTEPS, T);
        for (int k = 0; k < 8; k++) CHECK(P.begin(true) == PICK_NSTEPS, "pick %d after two misses checks", k);
        CHECK(P.begin(true) == 24, "the check after the 8 picks");
        // a miss, a settled outcome, a miss: no skip
        PickSettlePolicy Q;
        T = Q.begin(true), Q.outcome_sync(false, PICK_NSTEPS, T);
        T = Q.begin(true), Q.outcome_sync(true, 20, T);
        T = Q.begin(true), Q.outcome_sync(false, PICK_NSTEPS, T);
        CHECK(T == 20 && Q.begin(true) == 24 && Q.skip == 0, "misses that are not consecutive skip");
    }
    // SVTGPU_PICK_SETTLE=0: no check ever, whatever the state
    {
        PickSettlePolicy P;
        for (int k = 0; k < 30; k++) CHECK(P.begin(false) == PICK_NSTEPS, "a check with the checkpoint off");
    }
    // the documented difference: with `settle` below the clamp (a pick that settled at step 5) the synchronous miss
    // moves from the checkpoint used (16 -> 20), the asynchronous one from the word (5 -> 9, still clamped to 16)
    {
        PickSettlePolicy S, A;
        S.outcome_sync(true, 5, 24), A.outcome_async(true, 5);
        const int Ts = S.begin(true), Ta = A.begin(true);
        CHECK(Ts == 16 && Ta == 16, "T %d / %d after a settled outcome at 5", Ts, Ta);
        S.outcome_sync(false, PICK_NSTEPS, Ts), A.outcome_async(false, PICK_NSTEPS);
        CHECK(S.settle == 20 && A.settle == 9 && S.begin(true) == 20 && A.begin(true) == 16, "after a miss: settle %d / %d", S.settle, A.settle);
        // above the clamp the two agree, and both stop at NSTEPS - 4
        PickSettlePolicy S2, A2;
        S2.outcome_sync(true, 35, 36), A2.outcome_async(true, 35);
        const int T2 = S2.begin(true);
        A2.begin(true);
        S2.outcome_sync(false, PICK_NSTEPS, T2), A2.outcome_async(false, PICK_NSTEPS);
        CHECK(T2 == 35 && S2.settle == 36 && A2.settle == 36, "a miss at 35 moves to %d / %d", S2.settle, A2.settle);
    }
    return n;
}

// ---- the switches ----
static void check_knobs() {
    g_case = "knobs";
    PickKnobs k{};
    pick_knobs_read_process(k), pick_knobs_read_call(k); // the test runs this program without any SVTGPU_ variable
    CHECK(k.parts == 64 && k.chunk == PICK_CHUNK && k.settle && !k.stats && !k.persist && !k.async_steps, "defaults");
    const struct {
        const char *parts, *chunk, *settle, *persist, *fallback;
        int         want_parts, want_chunk;
        bool        want_settle, want_persist, want_steps;
    } cases[] = {{"7", "4", "0", "1", "steps", 7, 4, false, true, true},       {"256", "48", "1", "0", "persist", 256, 48, true, false, false},
                 {"0", "3", "", "", "", 64, PICK_CHUNK, true, false, false},    {"-5", "49", "00", "10", "step", 64, PICK_CHUNK, false, true, false},
                 {"x", "7", "no", "yes", "STEPS", 64, 4, true, false, false},   {"1", "47", "2", "2", "stepsx", 1, 44, true, false, false},
                 {"64", "13", "0x", "1x", "steps", 64, 12, false, true, true}};
    for (auto &c : cases) {
        setenv("SVTGPU_PICK_PARTS", c.parts, 1), setenv("SVTGPU_PICK_CHUNK", c.chunk, 1), setenv("SVTGPU_PICK_SETTLE", c.settle, 1);
        setenv("SVTGPU_PICK_PERSIST", c.persist, 1), setenv("SVTGPU_PICK_ASYNC_FALLBACK", c.fallback, 1), setenv("SVTGPU_PICK_STATS", "", 1);
        pick_knobs_read_process(k), pick_knobs_read_call(k);
        CHECK(k.parts == c.want_parts && k.chunk == c.want_chunk && k.settle == c.want_settle && k.persist == c.want_persist && k.async_steps == c.want_steps && k.stats,
              "PARTS=%s CHUNK=%s SETTLE=%s PERSIST=%s ASYNC_FALLBACK=%s: %d %d %d %d %d", c.parts, c.chunk, c.settle, c.persist, c.fallback, k.parts, k.chunk,
              k.settle, k.persist, k.async_steps);
        CHECK(k.chunk % 4 == 0 && k.chunk >= 4 && k.chunk <= PICK_CHUNK, "chunk %d", k.chunk);
    }
    // the per-process switches are read once, the per-call ones at every pick
    unsetenv("SVTGPU_PICK_PARTS"), unsetenv("SVTGPU_PICK_CHUNK"), unsetenv("SVTGPU_PICK_SETTLE"), unsetenv("SVTGPU_PICK_STATS");
    setenv("SVTGPU_PICK_PERSIST", "1", 1), unsetenv("SVTGPU_PICK_ASYNC_FALLBACK");
    const PickKnobs a = pick_knobs(); // the first read of the process
    setenv("SVTGPU_PICK_PARTS", "9", 1), setenv("SVTGPU_PICK_SETTLE", "0", 1), setenv("SVTGPU_PICK_PERSIST", "0", 1), setenv("SVTGPU_PICK_ASYNC_FALLBACK", "steps", 1);
    const PickKnobs b = pick_knobs();
    CHECK(a.parts == 64 && a.settle && a.persist && !a.async_steps, "the first read");
    CHECK(b.parts == 64 && b.settle && !b.persist && b.async_steps, "the second read: parts %d settle %d persist %d steps %d", b.parts, b.settle, b.persist, b.async_steps);
    for (const char *v : {"SVTGPU_PICK_PARTS", "SVTGPU_PICK_SETTLE", "SVTGPU_PICK_PERSIST", "SVTGPU_PICK_ASYNC_FALLBACK"}) unsetenv(v);
}

int main() {
    check_knobs();
    const long calls = check_schedule(), picks = check_tables(), layouts = check_layout(), policy = check_policy();
    if (g_fail) std::fprintf(stderr, "cdef_pick_plan_check: %d checks failed\n", g_fail);
    else
        std::printf("cdef_pick_plan_check ok: %ld scheduled calls, %zu tables (%ld settled and %ld unsettled chains, %ld settle checks that copy), "
                    "%ld picks against the oracle, %ld layouts, %ld policy picks\n",
                    calls, tables().size(), g_settled, g_unsettled, g_copies, picks, layouts, policy);
    return g_fail ? 1 : 0;
}
