// dlf_levels.h — the integer rules of the deblocking level search and level tables (dlf.hip), each stated once: the
// level of a (segment, reference, mode) class, which planes a trial or an apply filters, the bisection of
// search_filter_level as a resumable state machine, the device-resident form of the three searches and its plan, the
// picked levels, and the two environment switches.  No HIP runtime: a plain C++17 compiler builds it too
// (tests/dlf_levels_check.cpp); under hipcc the functions are __host__ __device__.  The kernels that run these rules
// are in dlf.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/svtgpu.h"

#ifdef __HIPCC__
#define DLF_HD __host__ __device__
#else
#define DLF_HD
#endif

namespace {

constexpr int MAX_TRIALS = 2; // levels per trial launch (the bisection's lo and hi candidates)
constexpr int MAX_JOBS   = 3; // planes per launch: the Y, U and V level searches run side by side

// the per-level thresholds (svt_aom_update_sharpness, EbDeblockingCommon.c:554-572): all a launch's arguments carry
struct LevelThresholds {
    uint8_t mblim[64], lim[64], hev[64];
};
// with the frame's level tables (svt_av1_loop_filter_frame_init, EbDeblockingCommon.c:76-139)
struct LevelTables : LevelThresholds {
    uint8_t lvl[3][2][128]; // [plane][dir][segment*16 + ref*2 + mode_lf]
};

DLF_HD inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the level of one (segment, reference, mode) class, cls = seg * 16 + ref * 2 + mode, of a plane and direction whose
// base level is lv (svt_av1_loop_filter_frame_init)
DLF_HD inline uint8_t level_entry(const SvtGpuLfParams &p, int pl, int dir, int lv, int cls) {
    const int feat[3][2] = {{1, 2}, {3, 3}, {4, 4}}; // SEG_LVL_ALT_LF_{Y_V, Y_H, U, V}
    const int seg = cls >> 4, ref = (cls >> 1) & 7, mode = cls & 1;
    int       ls  = lv;
    if (p.segmentation_enabled && p.seg_feature_enabled[seg][feat[pl][dir]])
        ls = clampi(ls + p.seg_feature_data[seg][feat[pl][dir]], 0, 63);
    int v = ls;
    if (p.mode_ref_delta_enabled) {
        const int scale = 1 << (ls >> 5);
        v = ls + p.ref_deltas[ref] * scale + (ref > 0 ? p.mode_deltas[mode] * scale : 0);
        v = clampi(v, 0, 63);
    }
    return (uint8_t)v;
}

DLF_HD inline void fill_level_table(const SvtGpuLfParams &p, int pl, int dir, int lv, uint8_t *out) {
    for (int cls = 0; cls < 128; cls++) out[cls] = level_entry(p, pl, dir, lv, cls);
}

// The rules about the frame's four levels take them as values -- y0 / y1: luma across vertical / horizontal edges, u,
// v -- so that a trial's levels need no copy of the parameters (on the device such a copy, its class deltas indexed
// per lane, lives in scratch memory).
// is the plane filtered at all with these levels (svt_aom_loop_filter_sb :575-582)
DLF_HD inline bool levels_active(int plane, int y0, int y1, int u, int v) {
    return plane == 0 ? (y0 || y1) : plane == 1 ? u != 0 : v != 0;
}
// the base level of a plane and direction
DLF_HD inline int levels_base(int plane, int d, int y0, int y1, int u, int v) {
    return plane == 0 ? (d == 0 ? y0 : y1) : plane == 1 ? u : v;
}
// Level k of the frame (0: y0, 1: y1, 2: u, 3: v; now `cur`) in a trial of `plane`'s search at lvl: try_filter_frame
// (:841-883) sets the searched plane's level -- of luma both directions (dir 2) or one (0 / 1) -- and leaves the others
DLF_HD inline int trial_level(int k, int plane, int dir, int lvl, int cur) {
    const bool set = plane == 0 ? (k == 0 ? dir != 1 : k == 1 && dir != 0) : k == plane + 1;
    return set ? lvl : cur;
}
DLF_HD inline bool plane_active(const SvtGpuLfParams &p, int plane) {
    return levels_active(plane, p.filter_level[0], p.filter_level[1], p.filter_level_u, p.filter_level_v);
}
DLF_HD inline int plane_level(const SvtGpuLfParams &p, int plane, int d) {
    return levels_base(plane, d, p.filter_level[0], p.filter_level[1], p.filter_level_u, p.filter_level_v);
}
DLF_HD inline void set_levels(SvtGpuLfParams &p, int y0, int y1, int u, int v) {
    p.filter_level[0] = y0, p.filter_level[1] = y1, p.filter_level_u = u, p.filter_level_v = v;
}
DLF_HD inline void set_trial_level(SvtGpuLfParams &p, int plane, int dir, int lvl) {
    set_levels(p, trial_level(0, plane, dir, lvl, p.filter_level[0]), trial_level(1, plane, dir, lvl, p.filter_level[1]),
               trial_level(2, plane, dir, lvl, p.filter_level_u), trial_level(3, plane, dir, lvl, p.filter_level_v));
}

inline void build_thresholds(int sh, LevelThresholds &L) {
    for (int l = 0; l < 64; l++) {
        int inside = l >> ((sh > 0) + (sh > 4));
        if (sh > 0) inside = std::min(inside, 9 - sh);
        inside     = std::max(inside, 1);
        L.lim[l]   = (uint8_t)inside;
        L.mblim[l] = (uint8_t)(2 * (l + 2) + inside);
        L.hev[l]   = (uint8_t)(l >> 4);
    }
}
inline void build_level_tables(const SvtGpuLfParams &p, LevelTables &L) {
    build_thresholds(p.sharpness_level, L);
    for (int pl = 0; pl < 3; pl++)
        for (int dir = 0; dir < 2; dir++) fill_level_table(p, pl, dir, plane_level(p, pl, dir), L.lvl[pl][dir]);
}

// Entry (d, cls) of the level table of one trial of `plane`'s search at `level`: the trial filters its plane alone --
// the other planes' levels do not gate it -- and a plane its levels leave off filters nothing: zero
DLF_HD inline uint8_t trial_level_entry(const SvtGpuLfParams &p, int plane, int search_dir, int level, int d, int cls) {
    const int y0 = trial_level(0, plane, search_dir, level, p.filter_level[0]);
    const int y1 = trial_level(1, plane, search_dir, level, p.filter_level[1]);
    const int u = trial_level(2, plane, search_dir, level, p.filter_level_u);
    const int v = trial_level(3, plane, search_dir, level, p.filter_level_v);
    return levels_active(plane, y0, y1, u, v) ? level_entry(p, plane, d, levels_base(plane, d, y0, y1, u, v), cls) : 0;
}

// Is `plane` filtered by an apply of the planes from plane_start on: its own levels, and luma off stops every plane
// of an apply that includes luma (svt_aom_loop_filter_sb :575-577; the loop starts at plane_start)
DLF_HD inline bool plane_filtered(const SvtGpuLfParams &p, int plane, int plane_start = 0) {
    return (plane_start > 0 || plane_active(p, 0)) && plane_active(p, plane);
}
// entry (d, cls) of the apply's level table of p's levels: zero for a plane that is not filtered
DLF_HD inline uint8_t apply_level_entry(const SvtGpuLfParams &p, int plane, int d, int cls, int plane_start = 0) {
    return plane_filtered(p, plane, plane_start) ? level_entry(p, plane, d, plane_level(p, plane, d), cls) : 0;
}

// the whole table [dir][class] of a trial / of the apply of planes from plane_start on (host)
inline void fill_trial_table(const SvtGpuLfParams &p, int plane, int search_dir, int level, uint8_t lvl[2][128]) {
    for (int d = 0; d < 2; d++)
        for (int cls = 0; cls < 128; cls++) lvl[d][cls] = trial_level_entry(p, plane, search_dir, level, d, cls);
}
inline void fill_apply_table(const SvtGpuLfParams &p, int plane, int plane_start, uint8_t lvl[2][128]) {
    for (int d = 0; d < 2; d++)
        for (int cls = 0; cls < 128; cls++) lvl[d][cls] = apply_level_entry(p, plane, d, cls, plane_start);
}

inline bool valid_params(const SvtGpuLfParams *p) {
    if (!p) return false;
    const int lv[4] = {p->filter_level[0], p->filter_level[1], p->filter_level_u, p->filter_level_v};
    for (int v : lv)
        if (v < 0 || v > 63) return false;
    return p->sharpness_level >= 0 && p->sharpness_level <= 7;
}

// search_filter_level (EbDeblockingFilter.c:886-991) as a resumable state machine: pending() names the levels the
// next step needs (advancing over steps whose levels are already known), feed() records their SSE.  Independent
// searches (U and V) then share launches.
struct LevelSearch {
    int     plane = 0, dir = 0, early_exit = 0, only4x4 = 0;
    int     mid = 0, step = 0, direction = 0, conv = 0, best = 0;
    int64_t best_err = 0, bias = 0, err[64];
    int     phase = 0; // 0: the start level; 1: bisection steps; 2: done
    int     lo = 0, hi = 0;
    bool    try_lo = false, try_hi = false;
    int     req[MAX_TRIALS], nreq = 0;

    DLF_HD LevelSearch() {}
    DLF_HD LevelSearch(const int last[4], int dlf_avg, int early_exit_, int only4x4_, int plane_, int dir_)
        : plane(plane_), dir(dir_), early_exit(early_exit_), only4x4(only4x4_) {
        const int start = plane == 0 ? (dlf_avg ? last[0] : last[dir]) : last[plane + 1];
        mid  = clampi(start, 0, 63);
        step = mid < 16 ? 4 : mid / 4;
        best = mid;
        for (int i = 0; i < 64; i++) err[i] = -1;
        req[0] = mid, nreq = 1;
    }
    // the next bisection step's candidates (try lo / hi around mid), or done
    DLF_HD void next_request() {
        if (step <= 0) {
            phase = 2, nreq = 0;
            return;
        }
        hi   = mid + step < 63 ? mid + step : 63, lo = mid - step > 0 ? mid - step : 0;
        bias = (best_err >> (15 - (mid / 8))) * step;
        if (!only4x4) bias >>= 1;
        try_lo = direction <= 0 && lo != mid, try_hi = direction >= 0 && hi != mid;
        nreq   = 0;
        if (try_lo) req[nreq++] = lo;
        if (try_hi) req[nreq++] = hi;
    }
    DLF_HD void resolve() {
        if (phase == 0) {
            best_err = err[mid], best = mid, phase = 1;
        } else {
            if (try_lo && err[lo] < best_err + bias) {
                if (err[lo] < best_err) best_err = err[lo];
                best = lo;
            }
            if (try_hi && err[hi] < best_err - bias) {
                best_err = err[hi];
                best     = hi;
            }
            if (best == mid) {
                conv++;
                step      = conv == early_exit ? 0 : step / 2;
                direction = 0;
            } else {
                direction = best < mid ? -1 : 1;
                mid       = best;
            }
        }
        next_request();
    }
    DLF_HD int pending(int *lv) {
        while (phase != 2) {
            int m = 0;
            for (int k = 0; k < nreq; k++) {
                bool dup = err[req[k]] >= 0;
                for (int j = 0; j < m && !dup; j++) dup = lv[j] == req[k];
                if (!dup) lv[m++] = req[k];
            }
            if (m) return m;
            resolve();
        }
        return 0;
    }
    DLF_HD void feed(const int *lv, int m, const unsigned long long *sse) {
        for (int k = 0; k < m; k++) err[lv[k]] = (int64_t)sse[k];
    }
};

// the levels and level tables of the next trial launch of the searches (on the device: written by the step from the
// previous launch's SSEs, no host decision between trials)
struct DlfDevPlan {
    int32_t ntrial[MAX_JOBS];                   // levels of each job in the next trial launch (0: the job has none)
    int32_t lv[MAX_JOBS][MAX_TRIALS];
    uint8_t lvl[MAX_JOBS][MAX_TRIALS][2][128];  // [job][trial][dir][class]
    int32_t done;                               // every search has finished
};

// The plane searches of one frame side by side (Y dir 2, then U and V), the parameters they started from and their
// next plan.  The host-driven search steps it on the host; the device-resident form (SVTGPU_DLF_DEVICE=1,
// svtgpu_dlf_pick_async) keeps it in HBM: after each trial launch one step feeds the SSEs to the searches and writes the
// next plan, so the bisection advances with no host decision between trials.  The host enqueues a chunk of (trial,
// step) pairs and reads the state back once per chunk; launches after the searches have finished find an empty plan
// (every workgroup returns at once).
struct DlfDevSearch {
    LevelSearch    srch[MAX_JOBS];
    int32_t        ns;
    SvtGpuLfParams p;
    DlfDevPlan     plan;
    int32_t        rounds; // trial rounds taken (svtgpu_dlf_pick_async)
};
// what an asynchronous search leaves for the apply (device) and the caller (mapped host memory)
struct DlfDevResult {
    int32_t levels[4]; // filter_level[0], [1], _u, _v
    int32_t rounds, seq, pad[2];
    uint8_t lvl[3][2][128]; // the apply's level tables of the picked levels (zero for a plane that is not filtered)
};

// the next launch's levels per search (the bisection steps)
DLF_HD inline void plan_levels(DlfDevSearch &S) {
    S.plan.done = 1;
    for (int i = 0; i < MAX_JOBS; i++) {
        const int m = i < S.ns ? S.srch[i].pending(S.plan.lv[i]) : 0;
        S.plan.ntrial[i] = m;
        if (m) S.plan.done = 0;
    }
}
// table entry e of [MAX_JOBS][MAX_TRIALS][2][128] (entries of levels the plan does not try are left as they are)
DLF_HD inline void plan_table_entry(DlfDevSearch &S, int e) {
    const int cls = e & 127, d = (e >> 7) & 1, k = (e >> 8) % MAX_TRIALS, i = (e >> 8) / MAX_TRIALS;
    if (i >= S.ns || k >= S.plan.ntrial[i]) return;
    S.plan.lvl[i][k][d][cls] = trial_level_entry(S.p, S.srch[i].plane, S.srch[i].dir, S.plan.lv[i][k], d, cls);
}
constexpr int PLAN_ENTRIES = MAX_JOBS * MAX_TRIALS * 2 * 128;
inline void plan_next(DlfDevSearch &S) { // host
    plan_levels(S);
    for (int e = 0; e < PLAN_ENTRIES; e++) plan_table_entry(S, e);
}

// The searches' start (LevelSearch's constructor: the start level) and the first plan's levels, from the frame's
// parameters; ns searches run (searches_for).  The tables follow (plan_table_entry).
DLF_HD inline void search_init(DlfDevSearch &S, const SvtGpuLfParams &p, int ns, int dlf_avg, int early_exit,
                               int only4x4) {
    const int last[4] = {p.filter_level[0], p.filter_level[1], p.filter_level_u, p.filter_level_v};
    const int dirs[MAX_JOBS] = {2, 0, 0};
    for (int i = 0; i < MAX_JOBS; i++) S.srch[i] = LevelSearch(last, dlf_avg, early_exit, only4x4, i, dirs[i]);
    S.ns = ns, S.p = p, S.rounds = 0;
    plan_levels(S);
}
// One bisection decision per search from the sums [MAX_JOBS][MAX_TRIALS] of the plan's trial launch, then the next
// plan's levels.  The tables follow (plan_table_entry).  A finished plan stays as it is: on the device dlf_step has
// returned before this call when the plan is done, so the first line only makes the function safe to call alone.
DLF_HD inline void search_step(DlfDevSearch &S, const unsigned long long *sums) {
    if (S.plan.done) return;
    for (int i = 0; i < S.ns; i++)
        if (S.plan.ntrial[i]) S.srch[i].feed(S.plan.lv[i], S.plan.ntrial[i], sums + i * MAX_TRIALS);
    plan_levels(S);
    S.rounds++;
}

// The searches a pick runs: with dlf_avg_uv on a non-base layer the chroma levels stay (EbDeblockingFilter.c:1221-1229)
DLF_HD inline int searches_for(int dlf_avg_uv, int temporal_layer_index) {
    return dlf_avg_uv && temporal_layer_index > 0 ? 1 : MAX_JOBS;
}
// The picked levels {filter_level[0], [1], _u, _v} (svt_av1_pick_filter_level): luma both directions from the dir-2
// search; chroma searched, or the levels the pick started from
DLF_HD inline void picked_levels(const LevelSearch *srch, int ns, const SvtGpuLfParams &start, int out[4]) {
    out[0] = out[1] = srch[0].best;
    out[2] = ns == MAX_JOBS ? srch[1].best : start.filter_level_u;
    out[3] = ns == MAX_JOBS ? srch[2].best : start.filter_level_v;
}

// The environment switches of the level search, read together once per process, at the first pick of either kind
// (dlf_knobs): measurements and tests set them.
struct DlfKnobs {
    // SVTGPU_DLF_DEVICE=0|1|n: (trial, step) pairs of the device search per host read-back, at most 64 (1: the default
    // chunk of 6); 0: the host-driven search; -1 (unset): chunk() decides
    int device_chunk;
    // SVTGPU_DLF_ROUNDS=k: the trial rounds svtgpu_dlf_pick_async enqueues, 1 .. 64 (tests: 1 makes the finish kernel
    // complete the search); 0 (unset): sized from the previous search
    int rounds;
    // Default: the device search for a tile of a picture spread over ranks (its trial launches are small, so the host
    // round trips and the all-reduce waits between them dominate: emulated 8-GPU rank 7.7-7.9 -> 8.1 Gpx/s), the
    // host-driven one for a whole picture (its launches sized per step beat the device plan's full-shape grid: 3053
    // vs 2949 Mpx/s)
    int chunk(bool tiled) const { return device_chunk >= 0 ? device_chunk : tiled ? 6 : 0; }
};
inline DlfKnobs dlf_knobs_read() {
    DlfKnobs    k;
    const char *e  = std::getenv("SVTGPU_DLF_DEVICE");
    k.device_chunk = e ? std::max(0, std::min(64, std::atoi(e) == 1 ? 6 : std::atoi(e))) : -1;
    e              = std::getenv("SVTGPU_DLF_ROUNDS");
    k.rounds       = e ? std::max(1, std::min(64, std::atoi(e))) : 0;
    return k;
}
inline const DlfKnobs &dlf_knobs() {
    static const DlfKnobs k = dlf_knobs_read();
    return k;
}

} // namespace
