// cdef_pick_plan.h — the integer rules of the frame-level CDEF strength pick (cdef_pick.hip), each stated once: the
// constants of its two kernels' shapes, the greedy schedule (which call of which chain a step makes), the layout of
// the pick's device and mapped buffers, the environment switches, the settle checkpoint's policy and index
// arithmetic, the RD choice over the strength count and the conversion of the chosen list into frame parameters.
// No HIP runtime: a plain C++17 compiler builds it too (tests/cdef_pick_plan_check.cpp); under hipcc the functions are
// __host__ __device__.  The kernels that run these rules, and the descriptions of them, are in cdef_pick.hip.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/svtgpu.h"

#ifdef __HIPCC__
#define PICK_HD __host__ __device__
#else
#define PICK_HD
#endif

// ---- constants ----
constexpr int PICK_NT         = 256; // lanes of a step or persistent workgroup
constexpr int PICK_MAX_CHAINS = 4;   // the greedy chains nb = 1, 2, 4, 8 (EbEncCdef.c:697-727)
constexpr int PICK_NSTEPS     = 40;  // calls of the longest chain: nb = 8 -> 8 + 32 (EbEncCdef.c:714-726)
constexpr int PICK_CHUNK      = 48;  // max FBs per step workgroup (their low words staged in LDS: <= 25.7 KB)
// LDS row of a staged FB (dwords): 128 entries + 4, so the per-FB best (a lane per FB reading its row) spreads over 8
// banks instead of one, and rows stay 16-B aligned for the accumulation's quad reads
constexpr int PICK_MROW = 132;
// the persistent kernel: PS_GRID resident workgroups = PS_NCH FB chunks (of <= PS_CH FBs) x 4 row groups; its exchange
// words carry an 8-bit tag above a 56-bit value
constexpr int                PS_GRID = 256;
constexpr int                PS_NCH  = 64;
constexpr int                PS_CH   = 32; // frames up to 2048 non-skipped 64x64 blocks (3840x2160: 2040)
constexpr unsigned long long PS_LOW  = (1ull << 56) - 1;

static_assert(PICK_NSTEPS == 5 * 8, "the longest chain (nb = 8) makes 5 nb calls");
static_assert((1 << (PICK_MAX_CHAINS - 1)) == 8 && PICK_MAX_CHAINS * 64 == PICK_NT, "a wave per chain");
static_assert(PS_GRID == 4 * PS_NCH, "a persistent workgroup per (chunk, row group)");
static_assert(PS_NCH % 4 == 0, "a row owner's four waves share the chunks' partial sums");
static_assert(PS_CH <= 64, "the persistent kernel's per-FB best: a lane per FB of the chunk");
static_assert(PICK_CHUNK % 4 == 0, "the accumulation takes four FBs per iteration");
static_assert(PICK_CHUNK * 32 / PICK_NT == 6 && PICK_CHUNK * 32 % PICK_NT == 0,
              "a step stages its chunk (32 uint4 per FB) through six registers per lane");
static_assert(PICK_MROW % 4 == 0 && PICK_MROW >= 128, "staged rows hold 128 entries and stay 16-B aligned");

// ---- the greedy schedule ----
// Chain c (nb = 1 << c strengths) makes 5 nb calls of svt_search_one_dual: nb growing calls with selection sizes
// 0 .. nb - 1, then 4 nb refinement calls of size nb - 1, each preceded by a shift of the selection (EbEncCdef.c:714-726).
PICK_HD inline int pick_chain_nb(int c) { return 1 << c; }
PICK_HD inline int pick_chain_calls(int c) { return 5 * pick_chain_nb(c); }

// Step s of the pick runs call s of every chain that still has one and folds the result of call s - 1 into the
// chain's selection.  One encoding, on the host and on the device, of what step `step` is for chain c:
//   nb_sel >= 0            live: this step makes a call with a selection of nb_sel entries
//   nb_sel == PICK_FINISH  the chain finishes with this step (step == 5 nb): the last call's result is folded in and
//                          the final list and value are published; no call
//   nb_sel == PICK_ENDED   the chain ended at an earlier step: nothing to do (so nb_sel < 0: no call at this step)
//   prev >= 0              the previous call's selection size: its result goes to slot prev (-1: no previous call)
//   shift                  ... and the selection is then shifted (this step's call is a refinement)
constexpr int PICK_FINISH = -1, PICK_ENDED = -2;
struct PickChainStep {
    int nb, nb_sel, prev, shift;
};
PICK_HD inline PickChainStep pick_chain_step(int c, int step) {
    const int     nb = pick_chain_nb(c), len = pick_chain_calls(c);
    PickChainStep r;
    r.nb     = nb;
    r.nb_sel = step > len ? PICK_ENDED : step < len ? (step < nb ? step : nb - 1) : PICK_FINISH;
    r.prev   = step == 0 || step > len ? -1 : (step - 1 < nb ? step - 1 : nb - 1);
    r.shift  = step >= 1 && step < len && step >= nb;
    return r;
}

// ---- records in the mapped pinned buffer ----
// the pick's result (pick_final_kernel)
struct PickOut {
    int32_t  sb_count, nbits, status, seq; // seq: the asynchronous pick that wrote it (0: a synchronous one)
    int32_t  gi[32]; // [0, 16) luma, [16, 32) chroma strength indices of the chosen list (zero past nb)
    uint64_t best[PICK_MAX_CHAINS];
};
// the settle check's outcome (pick_settle_kernel): settled = every unfinished chain settled, step = the latest step
// at which a chain that needs one settled (or finished)
struct SettleOut {
    int32_t settled, step, seq; // seq: the asynchronous pick that wrote it (its next T is read without a wait)
};

// ---- buffer layouts ----
// Every offset and size of the pick's buffers in SvtGpuCdefFrameState for a frame of nfb filter blocks: cdef_api.hip
// allocates and clears from it, cdef_pick.hip carves from it, cdef_apply.hip takes the device parameters' address.
struct PickLayout {
    // d_pick_part, 64-bit words: the compacted tables and the step kernels' accumulators
    size_t part_wmse;   // [nfb][2][64] compacted mse, bias applied
    size_t part_tot;    // [3][4][4096] rotating tot_mse accumulators
    size_t part_val;    // [NSTEPS + 1][4] value of the call before each step
    size_t part_wmse32; // [nfb][2][64] the low words of wmse, 32-bit (16-B aligned: the step kernel loads uint4)
    size_t part_words;  // the allocation
    // d_pick_lev, 32-bit words
    static constexpr size_t lev_lev   = 0;                                              // [NSTEPS + 1][4][32] selections
    static constexpr size_t lev_fin   = (size_t)(PICK_NSTEPS + 1) * PICK_MAX_CHAINS * 32; // [4][32] final lists
    static constexpr size_t lev_wide  = lev_fin + PICK_MAX_CHAINS * 32 + 33;              // the width flag
    static constexpr size_t lev_words = lev_fin + PICK_MAX_CHAINS * 32 + 64;
    // d_pick_out, 64-bit words: [4] value of each chain's last call
    static constexpr size_t out_words = 8;
    // d_fb_list, 32-bit words
    size_t list_fb;    // [nfb] the non-skipped FBs in raster order
    size_t list_count; // their count
    size_t list_inv;   // [nfb] FB -> its row in the compacted tables, or -1
    size_t list_words;
    // d_pick_xch, 64-bit words: the persistent kernel's exchange, then its status and diagnostics
    static constexpr size_t xch_part   = 0;                                          // [PS_NCH][4][4096] partial sums
    static constexpr size_t xch_amin   = (size_t)PS_NCH * PICK_MAX_CHAINS * 4096;    // [4][64][2] row minima
    static constexpr size_t xch_status = xch_amin + (size_t)PICK_MAX_CHAINS * 64 * 2; // int32: a poll gave up
    static constexpr size_t xch_stat   = xch_status + 8;                             // [4] diagnostics
    static constexpr size_t xch_words  = xch_status + 16;
    static constexpr size_t xch_bytes  = xch_words * 8;
    // d_apick, bytes (the asynchronous pick)
    static constexpr size_t apick_flag   = 0;  // int32: the settle check's settled word, read by the later steps
    static constexpr size_t apick_dep    = 8;  // uint32: the persistent fallback's epoch, counted on the device
    static constexpr size_t apick_params = 16; // SvtGpuCdefParams: what the apply reads
    static constexpr size_t apick_bytes  = 64;
    // h_pick, bytes (mapped pinned memory)
    static constexpr size_t rec_out    = 0;   // PickOut
    static constexpr size_t rec_settle = 448; // SettleOut
    static constexpr size_t rec_fbs    = 512; // [nfb] per-FB strength index
    size_t                  rec_bytes;

    explicit PickLayout(size_t nfb) {
        part_wmse   = 0;
        part_tot    = part_wmse + nfb * 128;
        part_val    = part_tot + (size_t)3 * PICK_MAX_CHAINS * 4096;
        part_wmse32 = part_val + (size_t)(PICK_NSTEPS + 1) * PICK_MAX_CHAINS;
        part_words  = part_wmse32 + nfb * 64;
        list_fb     = 0;
        list_count  = nfb;
        list_inv    = nfb + 1;
        list_words  = 2 * nfb + 1;
        rec_bytes   = rec_fbs + nfb;
    }
};
static_assert(PickLayout::rec_out + sizeof(PickOut) <= PickLayout::rec_settle, "PickOut fits below the settle record");
static_assert(PickLayout::rec_settle + sizeof(SettleOut) <= PickLayout::rec_fbs, "the settle record fits below the strengths");
static_assert(PickLayout::apick_params + sizeof(SvtGpuCdefParams) <= PickLayout::apick_bytes, "the device parameters fit");
static_assert(((size_t)3 * PICK_MAX_CHAINS * 4096 + (size_t)(PICK_NSTEPS + 1) * PICK_MAX_CHAINS) % 2 == 0,
              "wmse32 stays 16-B aligned behind the accumulators and values");
static_assert(PickLayout::lev_wide < PickLayout::lev_words, "the width flag lies in d_pick_lev");
#define SVTGPU_PICK_XCH_BYTES (PickLayout::xch_bytes)

// ---- launch shapes ----
// the persistent kernel holds a frame while its chunks hold every FB
inline bool ps_fits(int nfb) { return nfb <= PS_NCH * PS_CH; }
inline int  ps_chunk(int nfb) { return std::max(1, (nfb + PS_NCH - 1) / PS_NCH); } // FBs per chunk

// ---- environment switches ----
struct PickKnobs {
    // Read once per process, at the first pick (sweeps and measurements):
    int  parts;  // SVTGPU_PICK_PARTS=n: FB-chunk workgroups per step across the live chains (x 4 row tiles); default 64
    int  chunk;  // SVTGPU_PICK_CHUNK=n: FBs per step workgroup at most, 4 .. PICK_CHUNK rounded down to a multiple of 4
    bool settle; // SVTGPU_PICK_SETTLE=0: no settle checkpoint (every step launched)
    bool stats;  // SVTGPU_PICK_STATS set: the persistent kernel's per-phase ticks, to stderr
    // Read at every pick (tests and A/B runs change them between picks of one process):
    bool persist;     // SVTGPU_PICK_PERSIST=1: the persistent kernel (default: a launch per step)
    bool async_steps; // SVTGPU_PICK_ASYNC_FALLBACK=steps: the asynchronous pick's flagged step launches (default: one
                      // persistent fallback launch)
};
inline void pick_knobs_read_process(PickKnobs &k) {
    const char *e = std::getenv("SVTGPU_PICK_PARTS");
    k.parts       = e && std::atoi(e) > 0 ? std::atoi(e) : 64;
    e             = std::getenv("SVTGPU_PICK_CHUNK");
    const int c   = e ? std::atoi(e) : 0;
    k.chunk       = c >= 4 && c <= PICK_CHUNK ? c & ~3 : PICK_CHUNK;
    e             = std::getenv("SVTGPU_PICK_SETTLE");
    k.settle      = !(e && e[0] == '0');
    k.stats       = std::getenv("SVTGPU_PICK_STATS") != nullptr;
}
inline void pick_knobs_read_call(PickKnobs &k) {
    const char *e = std::getenv("SVTGPU_PICK_PERSIST");
    k.persist     = e && e[0] == '1';
    e             = std::getenv("SVTGPU_PICK_ASYNC_FALLBACK");
    k.async_steps = e && !std::strcmp(e, "steps");
}
// the switches of one pick
inline PickKnobs pick_knobs() {
    static const PickKnobs process = [] {
        PickKnobs k{};
        pick_knobs_read_process(k);
        return k;
    }();
    PickKnobs k = process;
    pick_knobs_read_call(k);
    return k;
}

// The shape of one step launch: ~256 workgroups per step whatever the number of live chains na (64 parts x 4 row
// tiles: 256 parts spent more on the u64 atomics than they gained, 0.66 -> 0.59 ms per pick + apply); more parts spread
// the accumulation, fewer mean fewer u64 atomics into the 4096 totals.  Shaped for every FB of the frame: the kernels
// read the non-skipped count on the device.
struct PickStepShape {
    int    chunk, parts, grid; // FBs per workgroup, FB chunks, workgroups = 4 row tiles x parts x na
    size_t lds;                // dynamic LDS: [chunk] staged rows + [chunk] 64-bit per-FB best
};
inline PickStepShape pick_step_shape(const PickKnobs &k, int nfb, int na) {
    PickStepShape sh;
    const int     want = std::max(1, k.parts / std::max(na, 1));
    sh.chunk = std::min(k.chunk, std::max(4, (nfb + want - 1) / std::max(want, 1)));
    sh.parts = std::max(1, (nfb + sh.chunk - 1) / sh.chunk);
    sh.grid  = 4 * sh.parts * na;
    sh.lds   = (size_t)sh.chunk * (PICK_MROW * 4 + 8);
    return sh;
}

// ---- the settle checkpoint's policy ----
// After step T of the launch path one small kernel checks whether every chain has settled into its period and, if so,
// writes the final lists, and the remaining launches are skipped (or return at once).  T follows the last pick's
// settling step; a check that finds a chain unsettled (a miss) moves it 4 steps later; after two consecutive misses
// the next 8 picks run without the check (its host wait saves nothing on a sequence that does not settle), then it is
// tried again from step 24.
struct PickSettlePolicy {
    int32_t settle = 24; // the step after which the next pick checks (clamped to 16 .. NSTEPS when used)
    int32_t miss   = 0;  // consecutive checks that found a chain unsettled
    int32_t skip   = 0;  // picks left that run without the check

    // At the start of a pick: the step T after which it checks, or PICK_NSTEPS: no check.
    int begin(bool settle_on) {
        const bool check = settle_on && skip == 0;
        if (skip > 0 && --skip == 0) settle = 24;
        return check ? std::min(std::max(settle, 16), PICK_NSTEPS) : PICK_NSTEPS;
    }
    // When a check's outcome is known.  The two callers differ in what a miss moves T from, because they differ in
    // when they learn the outcome:
    //  - the synchronous pick waits for its own check, made at T, so a miss moves to T + 4: from the checkpoint actually
    //    used, which is 16 when `settle` lay below the clamp;
    //  - the asynchronous pick takes the record of an earlier pick's check without a wait, at the start of a later
    //    pick (the host may run several picks ahead, and the record does not carry its T), so a miss moves to
    //    settle + 4: from the word as the records taken since have left it.  A `settle` below 16 therefore takes
    //    several misses to leave the clamp, and records skipped over (only the latest is seen) move nothing.
    void outcome_sync(bool settled, int step, int T) { outcome(settled, step, T); }
    void outcome_async(bool settled, int step) { outcome(settled, step, settle); }

private:
    void outcome(bool settled, int step, int from) {
        if (settled) {
            settle = step, miss = 0;
            return;
        }
        settle = std::min(from + 4, PICK_NSTEPS - 4); // keep checking: a later frame may settle
        if (++miss >= 2) skip = 8, miss = 0;
    }
};

// ---- the settle check's index arithmetic ----
// lev: [NSTEPS + 1][4][32] the selection entering each call ([0, 16) luma, [16, 32) chroma); val: [NSTEPS + 1][4] the
// value of the call before each step
PICK_HD inline size_t pick_lev_at(int s, int c, int i) { return ((size_t)s * PICK_MAX_CHAINS + c) * 32 + i; }
PICK_HD inline size_t pick_val_at(int s, int c) { return (size_t)s * PICK_MAX_CHAINS + c; }
// the state of chain c entering call s: entries [0, nb - 1) of both halves (the call appends entry nb - 1)
PICK_HD inline bool pick_same_state(const int32_t *lev, int c, int s1, int s2) {
    for (int q = 0; q < pick_chain_nb(c) - 1; q++)
        if (lev[pick_lev_at(s1, c, q)] != lev[pick_lev_at(s2, c, q)] ||
            lev[pick_lev_at(s1, c, 16 + q)] != lev[pick_lev_at(s2, c, 16 + q)])
            return false;
    return true;
}
// After step T's launch chain c (calls 0 .. L - 1, L = 5 nb) has either finished (L <= T) or entered call T with the
// selection lev[T].  A chain's refinement calls are a deterministic function of the state entering them, so once the
// state entering call s equals the one entering call s - nb (s - nb >= nb) the chain repeats with period nb from call
// s - nb on.  `at` is the first such s (L: the chain finishes first); seen at the checkpoint when at <= T.  A settled
// chain's last call L - 1 equals call a = T - nb + (L - 1 - T + nb) mod nb: the final list is lev[a] with slot nb - 1
// taken from lev[b] (b = the period twin of L: lev[t][nb - 1] is the result of call t - 1) and the value is val[a + 1]
// -- exactly what steps T + 1 .. L would produce.
struct PickSettle {
    int  at;       // the first repeating step, or L
    bool finished; // L <= T: the steps wrote the chain's final list and value
    bool settled;  // finished, or repeating by T
    int  a, b;     // settled and not finished: the steps whose lists give the final list; the value is val[a + 1]
    PICK_HD bool copies() const { return settled && !finished; } // the check writes the chain's final list and value
};
PICK_HD inline PickSettle pick_settle_chain(const int32_t *lev, int c, int T) {
    const int  nb = pick_chain_nb(c), L = pick_chain_calls(c);
    PickSettle r;
    r.at = L;
    for (int st = 2 * nb; st <= (T < L - 1 ? T : L - 1); st++)
        if (pick_same_state(lev, c, st, st - nb)) {
            r.at = st;
            break;
        }
    r.finished     = L <= T;
    r.settled      = r.finished || r.at <= T;
    r.a = r.b = -1;
    if (r.copies()) {
        const int base = T - nb;
        r.a = base + (L - 1 - base) % nb, r.b = base + (L - base) % nb;
    }
    return r;
}
// the final list and value of a chain that settled before it finished, as its remaining steps would have written them
PICK_HD inline void pick_settle_write(const int32_t *lev, const uint64_t *val, int c, const PickSettle &S, int32_t *fin,
                                      uint64_t *best) {
    const int nb = pick_chain_nb(c);
    for (int i = 0; i < 32; i++) fin[c * 32 + i] = lev[pick_lev_at(S.a, c, i)];
    fin[c * 32 + nb - 1]      = lev[pick_lev_at(S.b, c, nb - 1)];
    fin[c * 32 + 16 + nb - 1] = lev[pick_lev_at(S.b, c, 16 + nb - 1)];
    best[c]                   = val[pick_val_at(S.a + 1, c)];
}

// ---- RD choice over the number of signalled strengths (EbEncCdef.c:853-872) ----
struct PickChoice {
    int nbits, chain; // chain: the chosen chain (== nbits), or -1: no list chosen, the strengths stay zero
};
PICK_HD inline PickChoice pick_rd_choice(const uint64_t best[PICK_MAX_CHAINS], int sb_count, uint64_t lambda) {
    uint64_t   best_cost = (uint64_t)1 << 63;
    PickChoice r         = {0, -1};
    for (int i = 0; i < PICK_MAX_CHAINS; i++) {
        const int      nb   = pick_chain_nb(i);
        const int      bits = sb_count * i + nb * 6 * 2;
        const int64_t  rate = (int64_t)bits << 9;                                                              // av1_cost_literal
        const uint64_t cost = (uint64_t)(((rate * (int64_t)lambda + 256) >> 9) + ((int64_t)(best[i] * 16) << 7)); // RDCOST
        if (cost < best_cost) best_cost = cost, r.nbits = i, r.chain = i;
    }
    return r;
}
// the chosen list: gi[0, 16) luma, [16, 32) chroma strength indices, zero past nb; fin: [4][32] final list per chain
PICK_HD inline void pick_chosen_list(const int32_t *fin, PickChoice ch, int32_t gi[32]) {
    const int nb = 1 << ch.nbits;
    for (int j = 0; j < 16; j++) {
        gi[j]      = ch.chain >= 0 && j < nb ? fin[ch.chain * 32 + j] : 0;
        gi[16 + j] = ch.chain >= 0 && j < nb ? fin[ch.chain * 32 + 16 + j] : 0;
    }
}
// per-FB strength index (EbEncCdef.c:866-890): the first minimum over the chosen list; m0 / m1: the FB's luma /
// chroma rows of the compacted table
PICK_HD inline int pick_fb_strength(const uint64_t *m0, const uint64_t *m1, const int32_t *gi, int nb) {
    uint64_t bc = (uint64_t)1 << 63;
    int      bg = 0;
    for (int g = 0; g < nb; g++) {
        const uint64_t c = m0[gi[g]] + m1[gi[16 + g]];
        if (c < bc) bc = c, bg = g;
    }
    return bg;
}

// ---- the frame parameters of the chosen list ----
// strength index gi -> its code (filter_map, EbEncCdef.c:911-919), the damping (:921)
struct PickMap {
    uint8_t code[64];
    uint8_t damping;
};
inline PickMap pick_map_from(const SvtGpuCdefControls &ctrls, int32_t base_q_idx) {
    PickMap map;
    std::memset(&map, 0, sizeof map);
    const int nf = ctrls.first_pass_fs_num, end = nf + ctrls.default_second_pass_fs_num;
    for (int g = 0; g < end && g < 64; g++)
        map.code[g] = g < nf ? ctrls.default_first_pass_fs[g] : ctrls.default_second_pass_fs[g - nf];
    map.damping = (uint8_t)(3 + (base_q_idx >> 6));
    return map;
}
PICK_HD inline SvtGpuCdefParams pick_params_from(const PickMap &map, int nbits, const int32_t *gi) {
    SvtGpuCdefParams q;
    memset(&q, 0, sizeof q);
    q.cdef_damping = map.damping, q.cdef_bits = (uint8_t)nbits;
    for (int j = 0; j < (1 << nbits); j++)
        q.cdef_y_strength[j] = map.code[gi[j]], q.cdef_uv_strength[j] = map.code[gi[16 + j]];
    return q;
}
