// lr_plan.h — the host-side plan of the loop-restoration search (lr_search.hip): the environment knobs, the units and
// tiles of a band, the routing of every unit to the big or small instance of the two resident descents, and the
// layout of the search's device and pinned buffers.  Integer arithmetic only: no HIP runtime, so a plain C++17
// compiler builds it too (tests/lr_plan_check.cpp).  The kernels these declarations belong to, and the descriptions
// of them, are in lr_search.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/svtgpu.h"
#include "stage_layout.h"

#ifdef __HIPCC__
#define LR_HD __host__ __device__
#else
#define LR_HD
#endif

namespace {

struct Tile {
    int32_t plane, unit, x0, y0, w, h; // unit: global index over the searched planes
};
struct URect {
    int32_t h_start, h_end, v_start, v_end;
};

// ---- the resident Wiener descent (wiener_res_kernel, wiener_res_small_kernel) ----
constexpr int WR_NT = 1024, WR_RMAX = 32, WR_MAX_ROUNDS = 4096;
constexpr int WR_LDS_CAP = 152 * 1024; // largest CDEF window kept in LDS (bytes); larger units read global memory
constexpr int WRS_LDS_CAP = 38 * 1024; // ... of the small instance: four windows and the static words in a CU's 160 KB
constexpr int WRS_NT = 256, WRS_RMAX = 32;

// geometry of a unit in the lane layout: column-pair slots per segment (a multiple of 64), segments, rows per segment
struct WrGeo {
    int cpw, nseg, R;
};
LR_HD inline WrGeo wr_geo(int w, int h, int nt = WR_NT) { // nt: the instance's lanes
    WrGeo g;
    g.cpw  = (((w + 1) >> 1) + 63) & ~63;
    g.nseg = nt / g.cpw;
    g.R    = (h + g.nseg - 1) / g.nseg;
    return g;
}
LR_HD inline int wr_window_bytes(int w, int h) { return (h + 6) * ((w + 10) >> 1) * 4; }
// LDS mode: the window in LDS and the source rows in registers; else both are read from global memory per candidate
LR_HD inline bool wr_lds_mode(int w, int h, int lds_cap, int nt = WR_NT, int rmax = WR_RMAX) {
    const WrGeo g = wr_geo(w, h, nt);
    return wr_window_bytes(w, h) <= lds_cap && g.nseg > 0 && g.R <= rmax;
}
// A workgroup's share of a unit: rows [y0, y1) of unit `unit`.  A unit too large for one CU's LDS and registers (the
// frame's bottom unit row: 256 x 376 at 4K) is cut into `nparts` row parts on as many workgroups; each evaluates every
// candidate over its rows, the parts' SSEs meet through words in uncached memory (xch[2 * (first + part) + parity]:
// {round << 48 | partial SSE}, double-buffered by round parity), and every part takes the same descent step.  The
// parts of a unit are adjacent in the launch order and there are far fewer parted workgroups than CUs, so a waiting
// part's partner is always dispatched; the wait is bounded all the same (status bit 2).
struct WrItem {
    int32_t unit, y0, y1, part, nparts, first; // first: the item index of part 0 (exchange slots)
};
constexpr int WR_MAX_PARTS = 4;

// ---- the resident self-guided search (sgr_res_kernel, sgr_res_small_kernel) ----
#ifndef SVTGPU_SR_NT
#define SVTGPU_SR_NT 512
#endif
#ifndef SVTGPU_SR_KMAX
#define SVTGPU_SR_KMAX 19 // resident 4-pixel chunks per pixel lane: parts of <= 34048 pixels (256 x 133 luma)
#endif
constexpr int SR_NT = SVTGPU_SR_NT, SR_PW = SR_NT / 64 - 1, SR_PL = SR_PW * 64, SR_KMAX = SVTGPU_SR_KMAX;
constexpr int SR_LB = 4; // chunks whose loads are in flight together in the load phase
constexpr int SR_MAX_PX = SR_PL * SR_KMAX * 4;
constexpr int SR_MAX_PASSES = 4096, SR_MAX_PARTS = 8;
constexpr int sr_lds_bytes(int kmax) { return kmax * SR_PL * 8; } // the (x - src) pairs of the part
constexpr int SR_LDS = sr_lds_bytes(SR_KMAX);
// the small instance (sgr_res_small_kernel): one-part items of <= SRS_KMAX chunks per lane, SRS_WGS workgroups per CU
#ifndef SVTGPU_SRS_KMAX
#define SVTGPU_SRS_KMAX 10 // a 128 x 128 unit: 4096 chunks over 448 pixel lanes
#endif
#ifndef SVTGPU_SRS_WGS
#define SVTGPU_SRS_WGS 3 // 6 waves per SIMD: 80 VGPRs (at 4, 64 VGPRs, the load phase spilled 54-79 registers)
#endif
#ifndef SVTGPU_SRS_LB
#define SVTGPU_SRS_LB 1 // its load phase's group of chunks in flight (divides SR_LB: sr_pass reads whole groups of SR_LB)
#endif
constexpr int SRS_KMAX = SVTGPU_SRS_KMAX, SRS_WGS = SVTGPU_SRS_WGS, SRS_LDS = sr_lds_bytes(SRS_KMAX);
constexpr int SRS_LB = SVTGPU_SRS_LB;
static_assert(SR_LB % SRS_LB == 0, "the zero fill up to a multiple of SR_LB goes by load groups");
static_assert(SRS_KMAX <= SR_KMAX && SRS_WGS * (SRS_LDS + 2048) <= 160 * 1024, "SRS_WGS workgroups share a CU's LDS");
struct SrItem {
    int32_t pair, y0, y1, part, nparts, first; // rows [y0, y1) of the pair's unit; part q at grid position first + 8 q
};

// ---- the device RD finish (lr_fin_tables_kernel, lr_fin_walk_kernel) ----
constexpr int FIN_K1 = 63; // r = 1 / 2 masks: bit k < 63 = the unit k + 1 back as the reference, bit 63 = the default
constexpr int FIN_CH = 64; // the walks: units per chunk (a lane per unit; the switchable tables staged in LDS)
constexpr int FIN_OUT = 8; // device result words: frame types [3], search status, sequence

// The environment knobs of the search, read once per process (lr_knobs): measurements and tests set them.
struct LrKnobs {
    // largest Wiener window staged in LDS (SVTGPU_WR_LDS_CAP overrides: measurements of the global-memory path)
    int wr_lds_cap;
    bool wr_classic; // SVTGPU_WR_CLASSIC=1 (A/B): the round-4 Wiener step (thread 0, two barriers)
    // lanes of the small Wiener instance (wiener_res_small_kernel); 0: every unit on the big instance, which
    // SVTGPU_WR_CLASSIC=1 (thread 0's step: not in the small instance) and SVTGPU_WR_SMALL=0 (A/B, and the per-item
    // clocks of the small-size units there) ask for
    int wr_small_nt;
    // largest row part of the resident self-guided search (pixels); SVTGPU_SR_PART_PX lowers it (tests of the parted path)
    int sr_part_px;
    // candidates per pass of the resident self-guided search: a complete speculative tree of 1, 3 or 7 nodes
    // (SVTGPU_SR_TREE for A/B measurements).  One: the descent's own candidate sequence, 7.1 passes per (unit, ep) at 4K
    // against 3.9 (3 nodes) and 2.7 (7 nodes) -- the resident passes are cheap, and a larger tree's evaluated-but-unused
    // candidates cost the other frames' work at three frames in flight (2366 / 2321 Mpx/s for 1 / 3 nodes,
    // profiles/r03/srvar)
    int sr_tree_nodes;
    // SVTGPU_SR_1B=0 (A/B): every item on the two-barrier path, the control wave stepping the descent alone (round 3's form)
    bool sr_two_barriers;
    // whether small one-part items run on sgr_res_small_kernel: the default path only (one candidate per pass, one
    // barrier); SVTGPU_SR_SMALL=0 keeps every item on the big instance (A/B, and the per-item clocks of the small-size
    // items there)
    bool sr_small;
    // the self-guided row parts' exchange words: uncached memory (default) or, with SVTGPU_SR_XCH=l2, cached memory that
    // stays in the XCD's L2 (no memset: the search epoch tags the words)
    bool sr_l2;
    // SVTGPU_LR_FINISH=host: rest_finish_search on the host after a read-back of the records (the round-5 form; A/B)
    bool finish_on_host;
    bool timing;             // SVTGPU_LR_TIMING=1 prints the host-side phase times (wall clock, including the waits) to stderr
    bool wr_stats, sr_stats; // SVTGPU_WR_STATS / SVTGPU_SR_STATS: per-search diagnostics to stderr
    bool fin_clk;            // SVTGPU_LR_FIN_CLK: the device finish's phase clocks to stderr
    int  fin_win;            // SVTGPU_LR_FIN_WIN: the finish tables' window, 1 .. FIN_K1 (default)
    int  wn_prio;            // SVTGPU_WN_PRIO=0: the Wiener chain at normal priority (A/B)
};
inline LrKnobs lr_knobs_read() {
    auto is = [](const char *e, const char *v) { return e && !std::strcmp(e, v); };
    LrKnobs     k;
    const char *e     = std::getenv("SVTGPU_WR_LDS_CAP");
    k.wr_lds_cap      = e ? std::atoi(e) : WR_LDS_CAP;
    e                 = std::getenv("SVTGPU_WR_CLASSIC");
    k.wr_classic      = e && std::atoi(e) != 0;
    k.wr_small_nt     = k.wr_classic || is(std::getenv("SVTGPU_WR_SMALL"), "0") ? 0 : WRS_NT;
    e                 = std::getenv("SVTGPU_SR_PART_PX");
    k.sr_part_px      = e ? std::max(64, std::min(std::atoi(e), SR_MAX_PX)) : SR_MAX_PX;
    e                 = std::getenv("SVTGPU_SR_TREE");
    const int n       = e ? std::atoi(e) : 1;
    k.sr_tree_nodes   = n == 3 || n == 7 ? n : 1;
    k.sr_two_barriers = is(std::getenv("SVTGPU_SR_1B"), "0");
    k.sr_small        = !is(std::getenv("SVTGPU_SR_SMALL"), "0") && k.sr_tree_nodes == 1 && !k.sr_two_barriers;
    k.sr_l2           = is(std::getenv("SVTGPU_SR_XCH"), "l2");
    k.finish_on_host  = is(std::getenv("SVTGPU_LR_FINISH"), "host");
    k.timing          = std::getenv("SVTGPU_LR_TIMING") != nullptr;
    k.wr_stats        = std::getenv("SVTGPU_WR_STATS") != nullptr;
    k.sr_stats        = std::getenv("SVTGPU_SR_STATS") != nullptr;
    k.fin_clk         = std::getenv("SVTGPU_LR_FIN_CLK") != nullptr;
    e                 = std::getenv("SVTGPU_LR_FIN_WIN");
    k.fin_win         = e ? std::max(1, std::min(FIN_K1, std::atoi(e))) : FIN_K1;
    e                 = std::getenv("SVTGPU_WN_PRIO");
    k.wn_prio         = e ? std::atoi(e) : 1;
    return k;
}
inline const LrKnobs &lr_knobs() {
    static const LrKnobs k = lr_knobs_read();
    return k;
}

struct PlanePlan {
    int                  n = 0, nt = 0, unit_base = 0, tile_base = 0, win = 7, nval = 0, ne = 0, pair_base = 0;
    bool                 wn = false, sg = false;
    size_t               part_off = 0, mh_off = 0; // element offsets (int64)
    std::vector<int32_t> eps;
};

// plane p's Wiener window for the controls
inline int plane_win(const SvtGpuLrSearchControls *c, int p) {
    const int win_l = c->wn_filter_tap_lvl == 1 ? 7 : c->wn_filter_tap_lvl == 2 ? 5 : 3;
    return p == 0 ? win_l : std::min(win_l, 5);
}

// the units a search covers: unit rows [rb[p], re[p]) and unit columns [cb[p], ce[p]) of plane p
struct Band {
    int32_t rb[3], re[3], cb[3], ce[3];
};
// what a search plans from: the restored area, unit size and unit grid of every plane, the band, the planes searched
struct LrPlanIn {
    int32_t W[3], H[3], unit_size[3], hunits[3], vunits[3];
    Band    band;
    int32_t nplanes;
};

struct LrPlan {
    PlanePlan            pp[3];
    std::vector<URect>   units;
    std::vector<Tile>    tiles;
    std::vector<int32_t> tile0, uloc; // uloc: plane-local index of every global unit
    int                  npairs = 0, n_wn = 0, nt_wn = 0, n_sg = 0, nt_sg = 0, sg_planes = 0;
    size_t               flt_elems = 0, part_elems = 0, mh_elems = 0;
    // the records' layout: every plane's units back to back (the state's units, d_units[0]); dst[gu]: the record of
    // searched unit gu
    int32_t              nrec = 0, rbase[3] = {0, 0, 0};
    std::vector<int32_t> dst;
    std::vector<WrItem>  wr_items; // the big instance's items [0, n_wrb), then the small one's
    bool                 wr_parted = false;
    int                  wr_lds = 0, wrs_lds = 0, n_wrb = 0;
    std::vector<SrItem>  sr_items; // the big instance's grid [0, n_srb), then the small one's
    bool                 sr_parted = false;
    int                  n_srb = 0;
    int n_all() const { return (int)units.size(); }
    int nt_all() const { return (int)tiles.size(); }
    int n_wr() const { return (int)wr_items.size(); }
    int n_sr() const { return (int)sr_items.size(); }
};

// units (foreach_rest_unit_in_tile, EbRestoration.c:1257-1294), their <= 64x64 tiles, the eps
inline int lr_plan_units(LrPlan &plan, const LrPlanIn &in, const SvtGpuLrSearchControls *c) {
    const Band &b = in.band;
    for (int p = 0; p < in.nplanes; p++) {
        PlanePlan &q = plan.pp[p];
        const int  W = in.W[p], H = in.H[p], usz = in.unit_size[p], ext = usz * 3 / 2, off = 8 >> (p > 0);
        q.unit_base = (int)plan.units.size(), q.tile_base = (int)plan.tiles.size();
        int urow = 0, uidx = 0;
        for (int y0 = 0; y0 < H; urow++) {
            const int uh = (H - y0 < ext) ? H - y0 : usz;
            int       vs = std::max(0, y0 - off), ve = y0 + uh;
            if (ve < H) ve -= off;
            for (int x0 = 0, ucol = 0; x0 < W; uidx++, ucol++) {
                const int uw = (W - x0 < ext) ? W - x0 : usz;
                if (urow >= b.rb[p] && urow < b.re[p] && ucol >= b.cb[p] && ucol < b.ce[p]) {
                    plan.tile0.push_back((int)plan.tiles.size());
                    for (int y = vs; y < ve; y += 64)
                        for (int x = x0; x < x0 + uw; x += 64)
                            plan.tiles.push_back({p, (int)plan.units.size(), x, y, std::min(64, x0 + uw - x), std::min(64, ve - y)});
                    plan.units.push_back({x0, x0 + uw, vs, ve});
                    plan.uloc.push_back(uidx);
                }
                x0 += uw;
            }
            y0 += uh;
        }
        q.n = (int)plan.units.size() - q.unit_base, q.nt = (int)plan.tiles.size() - q.tile_base;
        if (urow != in.vunits[p] || uidx != in.hunits[p] * in.vunits[p]) return SVTGPU_ERR_INVALID_ARG;
        q.wn   = c->wn_enabled && (!p || c->wn_use_chroma);
        q.win  = plane_win(c, p);
        q.nval = (q.win * (q.win + 1) / 2 + 1) * 49;
        if (c->sg_enabled && (!p || c->sg_use_chroma))
            for (int e = c->sg_start_ep[p > 0]; e < c->sg_end_ep[p > 0]; e += std::max(1, c->sg_ep_inc[p > 0]))
                q.eps.push_back(e);
        q.ne = (int)q.eps.size(), q.sg = q.ne > 0;
        q.pair_base = plan.npairs;
        plan.npairs += q.n * q.ne;
        if (q.wn) {
            plan.n_wn += q.n, plan.nt_wn += q.nt;
            q.part_off = plan.part_elems, q.mh_off = plan.mh_elems;
            plan.part_elems += (size_t)q.nt * q.nval, plan.mh_elems += (size_t)q.n * q.nval;
        }
        if (q.sg) {
            plan.n_sg += q.n, plan.nt_sg += q.nt, plan.sg_planes++;
            plan.flt_elems += (size_t)(q.ne * 2 + 1) * ((W + 63) & ~63) * H; // the eps' g planes and the dx plane
        }
    }
    plan.tile0.push_back((int)plan.tiles.size());
    for (const Tile &t : plan.tiles) // 4-pixel chunks start on tile x offsets (unit columns: multiples of 32)
        if (t.x0 & 3) return SVTGPU_ERR_UNSUPPORTED;
    for (int p = 0; p < 3; p++) plan.rbase[p] = plan.nrec, plan.nrec += in.hunits[p] * in.vunits[p];
    plan.dst.resize(plan.n_all());
    for (int p = 0, gu = 0; p < in.nplanes; p++)
        for (int u = 0; u < plan.pp[p].n; u++, gu++) plan.dst[gu] = plan.rbase[p] + plan.uloc[gu];
    return SVTGPU_OK;
}

// The resident Wiener kernel takes every unit up to 384 columns wide (unit sizes <= 256): a unit is cut into the
// fewest row parts that fit one CU's LDS and registers each (global-memory mode when no cut up to WR_MAX_PARTS
// does); workgroups start with the largest parts (the longest chains), the parts of a unit adjacent.
// Each unit is routed by its own size: a one-part unit whose window and rows fit the small instance
// (wiener_res_small_kernel: several workgroups per CU) goes there, every other unit to the big one; wr_items holds
// the big instance's items, then the small one's, each largest first, and each launch's LDS is its own items' maximum
inline void lr_plan_wiener(LrPlan &plan, const LrKnobs &k) {
    const std::vector<URect> &units = plan.units;
    const int                 n_wn = plan.n_wn, wrs_nt = k.wr_small_nt, wrs_rmax = WRS_RMAX;
    std::vector<int> ord(n_wn);
    std::vector<int> np(n_wn, 1);
    std::vector<char> small(n_wn, 0);
    for (int u = 0; u < n_wn; u++) {
        const URect &r = units[u];
        const int    w = r.h_end - r.h_start, h = r.v_end - r.v_start;
        ord[u]         = u;
        int kp = 1;
        while (kp < WR_MAX_PARTS && !wr_lds_mode(w, (h + kp - 1) / kp, k.wr_lds_cap)) kp++;
        np[u] = wr_lds_mode(w, (h + kp - 1) / kp, k.wr_lds_cap) ? kp : 1;
        if (np[u] > 1) plan.wr_parted = true;
        const int hp = (h + np[u] - 1) / np[u];
        small[u]     = wrs_nt && np[u] == 1 && wr_lds_mode(w, h, std::min(WRS_LDS_CAP, k.wr_lds_cap), wrs_nt, wrs_rmax);
        if (small[u]) plan.wrs_lds = std::max(plan.wrs_lds, wr_window_bytes(w, h));
        else if (wr_lds_mode(w, hp, k.wr_lds_cap)) plan.wr_lds = std::max(plan.wr_lds, wr_window_bytes(w, hp));
    }
    auto part_area = [&](int u) {
        return (units[u].h_end - units[u].h_start) * ((units[u].v_end - units[u].v_start + np[u] - 1) / np[u]);
    };
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return part_area(a) > part_area(b); });
    for (int cls = 0; cls < 2; cls++) {
        for (int u : ord) {
            if (small[u] != cls) continue;
            const int h = units[u].v_end - units[u].v_start, first = (int)plan.wr_items.size();
            for (int kp = 0; kp < np[u]; kp++)
                plan.wr_items.push_back({u, h * kp / np[u], h * (kp + 1) / np[u], kp, np[u], first});
        }
        if (cls == 0) plan.n_wrb = (int)plan.wr_items.size();
    }
}

// The resident self-guided search (sgr_res_kernel): one item per (unit row part, ep).  Workgroups are dealt
// round-robin over the 8 XCDs (block b on XCD b mod 8), so the grid is laid out as 8 lanes (positions r, r + 8, ...):
// a unit's items -- its eps, and the row parts of each -- go to one lane, consecutively.  The eps of a unit then
// read its CDEF and source samples through one L2, and the parts of an item sit next to each other in their XCD's
// in-order dispatch, so a waiting part's partners are always dispatched after it (never behind other waiting
// parts).  Units are dealt largest first to the lane with the least work; empty slots (pair -1) pad the lanes.
// Each unit is routed by its own size: a one-part unit of at most SRS_KMAX chunks per lane goes to the small
// instance (sgr_res_small_kernel: more workgroups per CU), every other unit to the big one.  Each instance's grid
// has the 8-lane layout within itself; sr_items holds the big grid, then the small one (first: a position in the
// item's own grid -- the exchange words are the big instance's alone).
inline int lr_plan_sgr(LrPlan &plan, int nplanes, const LrKnobs &k) {
    if (!plan.npairs) return SVTGPU_OK;
    const std::vector<URect> &units = plan.units;
    const PlanePlan          *pp    = plan.pp;
    std::vector<std::vector<SrItem>> lanes[2] = {std::vector<std::vector<SrItem>>(8), std::vector<std::vector<SrItem>>(8)};
    std::vector<long long>           load[2] = {std::vector<long long>(8, 0), std::vector<long long>(8, 0)};
    std::vector<int>                 ord;
    for (int p = 0; p < nplanes; p++)
        if (pp[p].sg)
            for (int u = 0; u < pp[p].n; u++) ord.push_back(pp[p].unit_base + u);
    auto area = [&](int u) { return (long long)(units[u].h_end - units[u].h_start) * (units[u].v_end - units[u].v_start); };
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return area(a) > area(b); });
    for (int u : ord) {
        int p = 0;
        while (p + 1 < nplanes && u >= pp[p + 1].unit_base) p++;
        const PlanePlan &q = pp[p];
        const int        cw = (units[u].h_end - units[u].h_start + 3) >> 2, h = units[u].v_end - units[u].v_start;
        const int        maxrows = std::max(1, k.sr_part_px / 4 / std::max(cw, 1)), np = (h + maxrows - 1) / maxrows;
        if (np > SR_MAX_PARTS) return SVTGPU_ERR_UNSUPPORTED; // a unit wider than 1024 x 4 samples per row part
        plan.sr_parted |= np > 1;
        const int cls  = k.sr_small && np == 1 && (cw * h + SR_PL - 1) / SR_PL <= SRS_KMAX;
        const int lane = (int)(std::min_element(load[cls].begin(), load[cls].end()) - load[cls].begin());
        for (int e = 0; e < q.ne; e++) {
            const int first = (int)lanes[cls][lane].size(); // lane-local; made global below
            for (int part = 0; part < np; part++)
                lanes[cls][lane].push_back({q.pair_base + (u - q.unit_base) * q.ne + e, h * part / np,
                                            h * (part + 1) / np, part, np, first});
        }
        load[cls][lane] += area(u) * q.ne;
    }
    for (int cls = 0; cls < 2; cls++) {
        size_t len = 0;
        for (auto &l : lanes[cls]) len = std::max(len, l.size());
        const size_t base = plan.sr_items.size();
        plan.sr_items.resize(base + 8 * len, SrItem{-1, 0, 0, 0, 1, 0});
        for (int r = 0; r < 8; r++)
            for (size_t m = 0; m < lanes[cls][r].size(); m++) {
                SrItem it = lanes[cls][r][m];
                it.first  = 8 * it.first + r; // parts of an item: positions first, first + 8, ...
                plan.sr_items[base + 8 * m + r] = it;
            }
        if (cls == 0) plan.n_srb = (int)plan.sr_items.size();
    }
    return SVTGPU_OK;
}

// The plan of one search into an empty `plan`; an empty band leaves plan.units empty (nothing to search).
inline int lr_plan_build(LrPlan &plan, const LrPlanIn &in, const SvtGpuLrSearchControls &c, const LrKnobs &k) {
    if (int rc = lr_plan_units(plan, in, &c)) return rc;
    if (plan.units.empty()) return SVTGPU_OK;
    lr_plan_wiener(plan, k);
    return lr_plan_sgr(plan, in.nplanes, k);
}

// The search's device scratch (o_*: d_work), its uncached exchange arena (q_*) and its pinned staging (h_*).
// Three contiguous spans keep the host traffic to one copy each: the plan [0, plan_span) (uploaded when it changes),
// the accumulators [o_sum, o_sum + zero_span) zeroed per search, the results [o_sse, o_sse + res_span) read back
// (o_sse is the last zeroed and the first read).
struct LrLayout {
    size_t o_tiles, o_units, o_t0, o_witem, o_sritem, o_dst, plan_span;
    size_t o_sum, o_rec, o_path, o_sse, o_sse2, o_wstat, o_sstat, zero_span;
    size_t o_wu, o_wds, o_best, o_braw, res_span;
    size_t o_sds, o_part, o_mh, o_m1, o_m2, o_b1, o_b2, o_fout, work_bytes;
    size_t q_wrx, q_srx, qarena_bytes;
    size_t h_plan, h_res, h_cnt, h_out, h_rec, pin_bytes;
    // the host mirror of a member of the result span (the mirrors of the plan and result spans keep the device layout)
    size_t host(size_t o) const { return h_res + (o - o_sse); }
};
// descent_bytes: sizeof(Descent), the resumable descent the kernels keep per Wiener unit and per (unit, ep)
inline LrLayout lr_layout(const LrPlan &plan, size_t descent_bytes) {
    const int    n_all = plan.n_all(), nt_all = plan.nt_all(), n_wr = plan.n_wr(), n_sr = plan.n_sr();
    const int    n_wn = plan.n_wn, n_sg = plan.n_sg, nrec = plan.nrec;
    LrLayout     L;
    Carver       dc;
    L.o_tiles = dc(sizeof(Tile) * nt_all), L.o_units = dc(sizeof(URect) * n_all), L.o_t0 = dc(4 * (n_all + 1)),
    L.o_witem = dc(sizeof(WrItem) * (size_t)n_wr), L.o_sritem = dc(sizeof(SrItem) * (size_t)n_sr),
    L.o_dst = dc(4 * (size_t)n_all);
    L.plan_span = dc.off;
    // zeroed per search: the accumulators, the device finish's records (zero-padded: a tiled picture sums them) and
    // paths (a pass that does not run reads as "none taken")
    L.o_sum = dc(8 * n_all), L.o_rec = dc(sizeof(SvtGpuLrUnitSearch) * (size_t)nrec),
    L.o_path = dc(16 * (size_t)nrec), L.o_sse = dc(8 * n_all), L.o_sse2 = dc(8 * (size_t)n_sg), L.o_wstat = dc(8),
    L.o_sstat = dc(8);
    L.zero_span = dc.off - L.o_sum;
    L.o_wu = dc(sizeof(SvtGpuRestUnit) * n_wn), L.o_wds = dc(descent_bytes * n_wn),
    L.o_best = dc(16 * (size_t)n_sg), L.o_braw = dc(8 * (size_t)n_sg);
    L.res_span = dc.off - L.o_sse; // the (unit, ep) descents stay on the device: the best ep's come back
    L.o_sds = dc(descent_bytes * plan.npairs);
    L.o_part = dc(8 * plan.part_elems), L.o_mh = dc(8 * plan.mh_elems);
    L.o_m1 = dc(8 * (size_t)nrec), L.o_m2 = dc(8 * (size_t)nrec), L.o_b1 = dc(64 * (size_t)nrec),
    L.o_b2 = dc(64 * (size_t)nrec), L.o_fout = dc(4 * FIN_OUT);
    L.work_bytes = dc.off;
    // the uncached arena: the SSE exchange words of the Wiener units cut into row parts (wiener_res_kernel)
    Carver       qc;
    L.q_wrx = qc(16 * (size_t)n_wr), L.q_srx = qc(128 * (size_t)n_sr);
    L.qarena_bytes = qc.off;
    Carver       hc; // host mirrors of the plan and result spans keep the device layout
    L.h_plan = hc(L.plan_span), L.h_res = hc(L.res_span), L.h_cnt = hc(32), L.h_out = hc(sizeof(SvtGpuRestUnit) * n_all),
    L.h_rec = hc(sizeof(SvtGpuLrUnitSearch) * (size_t)nrec);
    L.pin_bytes = hc.off;
    return L;
}

} // namespace
