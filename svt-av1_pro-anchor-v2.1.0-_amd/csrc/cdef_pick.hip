// cdef_pick.hip — frame-level CDEF strength selection on the device.
//
// ≙ finish_cdef_search (Source/Lib/Encoder/Codec/EbEncCdef.c:728-926).  The expensive part is the
// 75 calls of svt_search_one_dual (:627-695): tot[j][k] = sum_fb min(best_fb, mse0[fb][j] +
// mse1[fb][k]) over 64x64 strength pairs, then the first minimum.  The four greedy chains
// (nb = 1, 2, 4, 8 → 5, 10, 20, 40 dependent calls, :697-727) are independent, so each device step
// advances every chain that is still running: step = one partial-sum kernel (FB chunks x chains)
// + one reduce/argmin kernel per chain that also appends the pick and pre-shifts the selection list
// for the next refinement call.  40 steps, all enqueued without host synchronisation (the grid is shaped
// for every FB; workgroups past the non-skipped count read on the device find no work).  The RD choice over
// nb (:853-872) and the per-FB assignment run on the device too and write the result straight into mapped
// pinned memory: one host synchronisation per pick.  The filter_map remap (:911-919) stays on the host.
// The integer rules -- the schedule, the buffer layouts, the switches, the settle policy and index arithmetic, the RD
// choice and the parameter conversion -- are in cdef_pick_plan.h (no HIP in it: tests/cdef_pick_plan_check.cpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "svtgpu_internal.h"

// the kernels' short names of the plan's constants
constexpr int NT = PICK_NT, MAX_CHAINS = PICK_MAX_CHAINS, NSTEPS = PICK_NSTEPS, MROW = PICK_MROW;

struct StepChain {
    int32_t chain;       // 0..3 (nb = 1 << chain)
    int32_t nb;
    int32_t nb_sel;      // selection size of this call (-1: finalize only)
    int32_t prev_nb_sel; // selection size of the previous call (-1: none)
    int32_t prev_shift;  // the previous call's result is followed by a refinement shift
};
struct StepArgs {
    const uint64_t *wmse;   // [sb_count][2][64] compacted, bias applied
    const uint32_t *wmse32; // the same entries' low words (what a step stages; the 64-bit path reads wmse)
    const int32_t  *count;  // sb_count, the number of non-skipped FBs (device)
    const int32_t  *wide;   // nonzero when some wmse entry is >= 2^31 (the 32-bit path would not be exact)
    int32_t         chunk, start_gi, end_gi, step, na; // na: chains in this launch
    int32_t         fb_alloc;                           // FB rows the wmse table holds
    uint64_t       *tot;    // [3][4][4096] rotating tot_mse accumulators
    int32_t        *lev;    // [NSTEPS+1][4][32] selection list entering each call
    int32_t        *fin;    // [4][32] final list per chain
    uint64_t       *best;   // [4] value returned by each chain's last call
    uint64_t       *val;    // [NSTEPS+1][4] value of the call before each step (the period shortcut's copy source)
    StepChain       ch[MAX_CHAINS];
    unsigned long long *wgclk; // diagnostics or null
    const int32_t  *skip;   // asynchronous pick, the steps after the settle check: nonzero = every chain settled, exit
};

// ---- compaction: non-skipped FBs in raster order, zero-strength bias (EbEncCdef.c:820-851) ----
__global__ void pick_compact_kernel(const uint8_t *skip, int nfb, int32_t *fb_list, int32_t *count, int32_t *wide,
                                    int32_t *fb_inv) {
    __shared__ int32_t base;
    __shared__ int32_t wsum[NT / 64];
    if (threadIdx.x == 0) base = 0, *wide = 0; // the gather raises the width flag
    __syncthreads();
    for (int c0 = 0; c0 < nfb; c0 += NT) {
        const int  fb   = c0 + threadIdx.x;
        const int  keep = fb < nfb && !skip[fb];
        const unsigned long long bal = __ballot(keep);
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const int pre  = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int i = 0; i < w; i++) off += wsum[i];
        if (keep) fb_list[off + pre] = fb;
        if (fb < nfb) fb_inv[fb] = keep ? off + pre : -1; // FB -> its row in the compacted tables
        __syncthreads();
        if (threadIdx.x == 0) base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

__global__ void pick_gather_kernel(const uint64_t *mse, int nfb, const int32_t *fb_list, const int32_t *count,
                                   int bias, uint64_t *wmse, uint32_t *wmse32, int32_t *wide, uint64_t *tot0) {
    const int i = blockIdx.x;
    if (tot0) // the first step's accumulators (launch path), spread over the grid
        for (int e = i * 128 + threadIdx.x; e < MAX_CHAINS * 4096; e += gridDim.x * 128) tot0[e] = 0;
    if (i >= *count) return;
    const int fb = fb_list[i];
    const int p = threadIdx.x >> 6, g = threadIdx.x & 63; // 128 threads
    uint64_t  v = mse[((size_t)p * nfb + fb) * 64 + g];
    if (bias && g == 0) v = ((uint64_t)bias * v) >> 6;
    wmse[((size_t)i * 2 + p) * 64 + g]   = v;
    wmse32[((size_t)i * 2 + p) * 64 + g] = (uint32_t)v;
    if (__any(v >> 31)) // m0 + m1 may leave 32 bits: the step kernels keep the 64-bit arithmetic
        if ((threadIdx.x & 63) == 0) atomicOr(wide, 1);
}

// First minimum of tot over [start, end)^2 (svt_search_one_dual's final loop, EbEncCdef.c:670-679),
// computed by every workgroup that needs it from the lane's 16 entries tv[u] = tot[u * NT + t] (loaded by the caller
// at the top of the step).  Returns (best, e = j*64 + k) through LDS.
__device__ __forceinline__ void tot_argmin(const uint64_t (&tv)[4096 / NT], int start, int end, uint64_t *bv, int32_t *bi) {
    const int t    = threadIdx.x;
    uint64_t  best = (uint64_t)1 << 63; // best_tot_mse initial value (EbEncCdef.c:632)
    int       idx  = 1 << 30;
#pragma unroll
    for (int u = 0; u < 4096 / NT; u++) { // ascending e per lane keeps the first minimum
        const int      e = u * NT + t, j = e >> 6, k = e & 63;
        const uint64_t v = tv[u];
        if (j >= start && j < end && k >= start && k < end && v < best) {
            best = v;
            idx  = e;
        }
    }
    // (value, index) minimum over the wave with cross-lane shuffles, then over the 4 waves: 2 barriers instead of 8
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ov = __shfl_xor(best, o);
        const int      oi = __shfl_xor(idx, o);
        if (ov < best || (ov == best && oi < idx)) best = ov, idx = oi;
    }
    if ((t & 63) == 0) bv[t >> 6] = best, bi[t >> 6] = idx;
    __syncthreads();
    if (t == 0)
        for (int w = 1; w < NT / 64; w++)
            if (bv[w] < bv[0] || (bv[w] == bv[0] && bi[w] < bi[0])) bv[0] = bv[w], bi[0] = bi[w];
    __syncthreads();
}

// One launch per greedy step: every active chain finishes its previous svt_search_one_dual call
// (argmin of the previous tot), forms the selection entering this call (append + refinement shift,
// EbEncCdef.c:714-726) and accumulates this call's tot[j][k] = sum_fb min(best_fb, m0[j] + m1[k]).
// grid (4 tiles of 16 rows j, FB chunks, chains).  The chunk's mse rows are staged in LDS; lane
// k = t & 63, wave q owns rows 16*tile + 4*q + {0..3}; partials meet through u64 atomics.
__global__ void __launch_bounds__(NT) sod_step_kernel(const StepArgs A) {
    // [chunk][128] low words of the mse rows + [chunk] best (half the 64-bit rows): when other frames' kernels hold
    // most of a CU's LDS, a step's workgroups find room beside them
    extern __shared__ __attribute__((aligned(16))) uint64_t dyn[];
    const uint32_t *m32 = (const uint32_t *)dyn; // entry e of FB f of the chunk at m32[f * MROW + e]
    __shared__ uint64_t bv[NT / 64];
    __shared__ int32_t  bi[NT / 64];
    __shared__ int32_t  sl[32];
    // 1-D grid of 4 row tiles x parts x chains, ordered part-major on the logical index and placed so that
    // consecutive logical indices share an XCD: the 4 * na workgroups staging one FB chunk read it through one L2
    if (A.skip && *A.skip) return; // uniform: the settle check wrote the final lists (svtgpu_cdef_pick_async)
    wgclk_mark(A.wgclk, 0);
    const int li = xcd_swizzle(blockIdx.x, gridDim.x), tx = li & 3, tz = (li >> 2) % A.na, ty = (li >> 2) / A.na;
    const int nparts = gridDim.x / (4 * A.na);
    const StepChain C = A.ch[tz];
    const int t = threadIdx.x, c = C.chain;
    const int lead = tx == 0 && ty == 0;
    if (C.nb_sel < 0 && !lead) return; // finalize-only entry: one workgroup
    const int f0 = ty * A.chunk;
    uint64_t *sbest = dyn + (size_t)A.chunk * (MROW / 2);
    // the period shortcut.  A chain's refinement calls (EbEncCdef.c:714-726) are a deterministic function of the
    // ordered selection entering them (entries [0, nb - 1) of lev[s]); once the selection entering call s equals the
    // one entering call s - nb, calls s, s + 1, ... repeat calls s - nb, ... result for result (the greedy loop has
    // settled into re-adding what it drops), so they are copied instead of recomputed: every workgroup reads the same
    // two lists and makes the same decision.  lp = lev[s - 1 - nb] (the previous call's period twin), lr = lev[s - nb]
    // (whose slot nb - 1 holds the twin's result).  These loads go first: a repeat is known as soon as they land, and
    // then only the chain's lead workgroup stays (to write the step's list and value; no other has work)
    const int s = A.step, nb = C.nb;
    int       lcur = 0, lp = 0, lr = 0;
    const bool chk_prev = C.prev_nb_sel >= 0 && s - 1 - nb >= nb, chk_cur = C.nb_sel >= 0 && s - nb >= nb;
    if ((t & 63) < 32) {
        if (chk_prev) {
            lcur = A.lev[((size_t)(s - 1) * MAX_CHAINS + c) * 32 + (t & 31)];
            lp   = A.lev[((size_t)(s - 1 - nb) * MAX_CHAINS + c) * 32 + (t & 31)];
        }
        if (chk_prev || chk_cur) lr = A.lev[((size_t)(s - nb) * MAX_CHAINS + c) * 32 + (t & 31)];
    }
    // 0. then every other global load of the step, issued before anything waits on one: the previous call's totals, this
    // workgroup's FB chunk (clamped into the allocated table, not the live count, so no load waits for the count)
    // and the live count and width flag.  The chunk (its low words: half the bytes of the 64-bit rows) stays in named
    // registers (not an array: VGPRs, not scratch) through the argmin and lands in LDS after it
    uint64_t tv[4096 / NT];
    {
        const uint64_t *tot = A.tot + ((size_t)((A.step + 2) % 3) * MAX_CHAINS + c) * 4096;
#pragma unroll
        for (int u = 0; u < 4096 / NT; u++) tv[u] = C.prev_nb_sel >= 0 ? tot[u * NT + t] : 0;
    }
    static_assert(PICK_CHUNK * 32 / NT == 6, "six staging registers per lane");
    const uint4 *src = (const uint4 *)(A.wmse32 + (size_t)f0 * 128);
    const int    lim = min(A.chunk, A.fb_alloc - f0) * 32 - 1; // f0 < fb_alloc: the grid covers the table
#define LD(u) const uint4 v##u = src[min(t + (u) * NT, lim)];
    LD(0) LD(1) LD(2) LD(3) LD(4) LD(5)
#undef LD
    const int  nfb  = C.nb_sel < 0 ? 0 : min(*A.count - f0, A.chunk);
    const int  wide = *A.wide;
    const bool in_state = (t & 15) < nb - 1 && (t & 63) < 32; // lanes holding entries [0, nb - 1) of both halves
    const bool prev_rep = chk_prev && !__ballot(in_state && lcur != lp);
    if (prev_rep && !lead) return; // a repeated previous call makes this one a repeat too
    wgclk_mark(A.wgclk, 1);
    // 1. selection entering this call
    if (t < 32) sl[t] = A.step ? A.lev[((size_t)(A.step - 1) * MAX_CHAINS + c) * 32 + t] : 0;
    if (C.prev_nb_sel >= 0) {
        uint64_t pv;
        int      pj, pk;
        if (prev_rep) { // the previous call repeated its twin: the twin's result and value
            pj = __shfl(lr, nb - 1), pk = __shfl(lr, 16 + nb - 1);
            pv = A.val[(size_t)(s - nb) * MAX_CHAINS + c];
        } else {
            tot_argmin(tv, A.start_gi, A.end_gi, bv, bi);
            const bool any = bi[0] < (1 << 30); // no candidate: (1 << 63, 0, 0) like the reference
            pj = any ? bi[0] >> 6 : 0, pk = any ? bi[0] & 63 : 0;
            pv = any ? bv[0] : ((uint64_t)1 << 63);
        }
        if (t == 0) {
            sl[C.prev_nb_sel]      = pj;
            sl[16 + C.prev_nb_sel] = pk;
            if (C.prev_shift)
                for (int q = 0; q < C.nb - 1; q++) {
                    sl[q]      = sl[q + 1];
                    sl[16 + q] = sl[16 + q + 1];
                }
            if (lead) A.val[(size_t)s * MAX_CHAINS + c] = pv;
            if (lead && C.nb_sel < 0) A.best[c] = pv;
        }
    }
    if (nfb > 0) {
        uint4 *dst = (uint4 *)dyn; // the low words (the 64-bit path reads the table itself), rows MROW dwords apart
#define ST(u) \
    if (t + (u) * NT < nfb * 32) dst[((t + (u) * NT) >> 5) * (MROW / 4) + ((t + (u) * NT) & 31)] = v##u;
        ST(0) ST(1) ST(2) ST(3) ST(4) ST(5)
#undef ST
    }
    __syncthreads();
    if (C.nb_sel < 0) { // the chain's last call has finished: publish its list
        if (t < 32) A.fin[c * 32 + t] = sl[t];
        return;
    }
    wgclk_mark(A.wgclk, 2);
    if (lead && t < 32) A.lev[((size_t)A.step * MAX_CHAINS + c) * 32 + t] = sl[t];
    // this call repeats its twin: nothing to accumulate (nor to zero: the chain's later calls repeat too)
    if (chk_cur && !__ballot(in_state && sl[t & 31] != lr)) return;
    // 2. zero this workgroup's slice of the accumulator used by the next step
    {
        uint64_t *nxt = A.tot + ((size_t)((A.step + 1) % 3) * MAX_CHAINS + c) * 4096;
        const int nwg = 4 * nparts, wg = ty * 4 + tx;
        for (int e = wg * NT + t; e < 4096; e += nwg * NT) nxt[e] = 0;
    }
    if (nfb <= 0) return;
    // 3. per-FB best over the selection (EbEncCdef.c:645-651)
    const uint64_t *gm = A.wmse + (size_t)f0 * 128; // the chunk's full entries (64-bit path)
    if (t < nfb) {
        uint64_t b = (uint64_t)1 << 63;
        for (int g = 0; g < C.nb_sel; g++) {
            const uint64_t v = wide ? gm[t * 128 + sl[g]] + gm[t * 128 + 64 + sl[16 + g]]
                                    : (uint64_t)m32[t * MROW + sl[g]] + m32[t * MROW + 64 + sl[16 + g]];
            b = v < b ? v : b;
        }
        sbest[t] = b;
    }
    __syncthreads();
    wgclk_mark(A.wgclk, 3);
    // 4. accumulate.  When every entry is < 2^31 (the usual case: the check is in pick_gather_kernel), m0 + m1
    // and the min stay in 32 bits and only the running sum is 64-bit: 4 ALU ops per term instead of 7
    const int k = t & 63, j0 = 16 * tx + 4 * (t >> 6);
    uint64_t  acc[4] = {0, 0, 0, 0};
    if (!wide) {
        auto term = [&](int f) {
            const uint64_t b64 = sbest[f];
            const uint32_t b = b64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b64, m1k = m32[f * MROW + 64 + k];
            const uint4    m0 = *(const uint4 *)&m32[f * MROW + j0]; // j0 and MROW are multiples of 4
            acc[0] += min(m0.x + m1k, b), acc[1] += min(m0.y + m1k, b);
            acc[2] += min(m0.z + m1k, b), acc[3] += min(m0.w + m1k, b);
        };
        int f = 0;
        for (; f + 4 <= nfb; f += 4) { // 4 FBs per iteration: their LDS reads issue together
#pragma unroll
            for (int q = 0; q < 4; q++) term(f + q);
        }
        for (; f < nfb; f++) term(f);
    } else {
        for (int f = 0; f < nfb; f++) { // entries >= 2^31 somewhere in the frame: the full entries from the table
            const uint64_t b = sbest[f], m1k = gm[f * 128 + 64 + k];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t v = gm[f * 128 + j0 + u] + m1k;
                acc[u] += v < b ? v : b;
            }
        }
    }
    wgclk_mark(A.wgclk, 4);
    uint64_t *cur = A.tot + ((size_t)(A.step % 3) * MAX_CHAINS + c) * 4096;
    if (k >= A.start_gi && k < A.end_gi)
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (j0 + u >= A.start_gi && j0 + u < A.end_gi)
                atomicAdd((unsigned long long *)&cur[(j0 + u) * 64 + k], (unsigned long long)acc[u]);
    if (A.wgclk) {
        __syncthreads();
        wgclk_mark(A.wgclk, 5);
    }
}

// ---- the same greedy chains in one persistent launch ----
// PS_GRID workgroups stay resident for all NSTEPS + 1 steps: workgroup (chunk ci, row group g) keeps FB chunk ci
// (<= PS_CH FBs) in LDS from the first step to the last and accumulates rows 16 g .. 16 g + 15 of every live chain's
// tot over it.  A step is two exchanges through tagged 64-bit words (an 8-bit tag of the pick and step above a
// 56-bit value, stored and polled with agent-scope atomics: a word is valid by itself, no fence or counter):
//   1. the partial sums of every chunk -> the workgroup that owns row j of chain c sums its 64 entries over the 64
//      chunks and publishes the row's first minimum (value, index);
//   2. every workgroup reads the rows' minima of every live chain and takes the first minimum of the call
//      (svt_search_one_dual's final loop, EbEncCdef.c:670-679), which every workgroup folds into the same selection.
// The words of one exchange are rewritten at every step before anyone can read the next step's (a workgroup
// reaches step s + 1 only after every row owner has read step s), so one buffer serves all steps; the pick's
// 2-bit epoch in the tag keeps the previous pick's words apart.  Co-residency: PS_GRID workgroups of <= 34 KB
// LDS and 256 threads (several fit per CU, and a pick launched beside another finds room); a poll gives up after
// a bounded wait and sets a status bit, so a grid that cannot drain still ends.  Partial sums fit 56 bits:
// an entry is < 2^41 (a 64x64 block's SSE at 12 bits is < 2^37), a chunk sums <= PS_CH of them, a total <= 2^15.
// (PS_GRID, PS_NCH, PS_CH and the tag mask PS_LOW: cdef_pick_plan.h)
struct PersistArgs {
    const uint64_t     *wmse;   // [fb_alloc][2][64] compacted, bias applied
    const int32_t      *count;  // live FB count (device)
    const int32_t      *wide;   // some entry >= 2^31: 64-bit terms
    int32_t             chunk, fb_alloc, end_gi;
    uint32_t            epoch;  // low 2 bits tag this pick's words
    unsigned long long *part;   // [PS_NCH][4][4096] tagged partial sums
    unsigned long long *amin;   // [4][64][2] tagged row minima: value, index
    int32_t            *fin;    // [4][32] final list per chain
    uint64_t           *best;   // [4]
    int32_t            *status; // bit 0: a poll gave up
    unsigned long long *stat;   // diagnostics (SVTGPU_PICK_STATS) or null: ticks of compute, exchange 1, exchange 2
    const int32_t      *skip;   // the asynchronous pick's fallback: nonzero = every chain settled at the check, exit
    const uint32_t     *dep;    // ... its epoch, counted on the device (the check raises it when this launch will run)
};

// poll the N tagged words p[i * stride] (those with use set) until every tag matches; false after the bounded wait
template <int N>
__device__ __forceinline__ bool ps_poll(const unsigned long long *p, size_t stride, bool use, unsigned long long (&v)[N],
                                        unsigned long long tag) {
    if (!use) return true;
    uint32_t pend = (1u << N) - 1; // words still to see: a re-poll loads only those
    for (unsigned spin = 0;; spin++) {
#pragma unroll
        for (int i = 0; i < N; i++)
            if (pend >> i & 1) {
                v[i] = __hip_atomic_load(p + i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((v[i] & ~PS_LOW) == tag) pend &= ~(1u << i);
            }
        if (!pend) return true;
        if (spin > (1u << 20)) return false; // ~0.1 s
        __builtin_amdgcn_s_sleep(4);
    }
}

// the sum of the N tagged words p[i * stride] (their 56-bit values), each added once its tag is seen
template <int N>
__device__ __forceinline__ bool ps_poll_sum(const unsigned long long *p, size_t stride, unsigned long long tag,
                                            unsigned long long &sum) {
    uint32_t pend = (1u << N) - 1;
    sum           = 0;
    for (unsigned spin = 0;; spin++) {
#pragma unroll
        for (int i = 0; i < N; i++)
            if (pend >> i & 1) {
                const unsigned long long v = __hip_atomic_load(p + i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((v & ~PS_LOW) == tag) pend &= ~(1u << i), sum += v & PS_LOW;
            }
        if (!pend) return true;
        if (spin > (1u << 20)) return false; // ~0.1 s
        __builtin_amdgcn_s_sleep(4);
    }
}

__device__ __forceinline__ void ps_store(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(NT, 4) sod_persist_kernel(const PersistArgs A) {
    __shared__ __attribute__((aligned(16))) uint64_t m64[PS_CH * 128]; // the chunk: u64 rows, or u32 rows (narrow)
    __shared__ uint64_t sb[MAX_CHAINS][PS_CH];                          // per-FB best over each chain's selection
    __shared__ int32_t  sl[MAX_CHAINS][32];                             // selections ([0,16) luma, [16,32) chroma)
    __shared__ uint64_t red[NT];
    __shared__ int      s_fail;
    const uint32_t *m32 = (const uint32_t *)m64;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int li = xcd_swizzle(blockIdx.x, gridDim.x), ci = li >> 2, g = li & 3; // a chunk's 4 groups share an XCD
    const int f0 = ci * A.chunk, end = A.end_gi;
    const int nfb  = max(0, min(*A.count - f0, A.chunk));
    const int wide = *A.wide;
    if (A.skip && *A.skip) return; // uniform: the settle check finished the pick (svtgpu_cdef_pick_async)
    const unsigned long long ep = (unsigned long long)((A.dep ? *A.dep : A.epoch) & 3) << 62;
    unsigned long long       tk[3] = {0, 0, 0}, t0 = 0;
    if (t == 0) s_fail = 0;
    // the chunk into LDS, once (narrow: the low words, entry e of FB f at m32[f * 128 + e])
    for (int e = t; e < nfb * 128; e += NT) {
        const uint64_t v = A.wmse[(size_t)f0 * 128 + e];
        if (wide) m64[e] = v;
        else ((uint32_t *)m64)[e] = (uint32_t)v;
    }
    if (t < MAX_CHAINS * 32) sl[t >> 5][t & 31] = 0;
    __syncthreads();
    for (int step = 0; step <= NSTEPS; step++) {
        const unsigned long long tag = ep | (unsigned long long)(step + 1) << 56, ptag = ep | (unsigned long long)step << 56;
        if (A.stat && t == 0) t0 = __builtin_amdgcn_s_memrealtime();
        // 1. the previous call's first minimum per chain (wave c: lane j holds row j's minimum), folded into the
        // selection; a finishing chain publishes its list and value
        {
            const int       c = w;
            const PickChainStep C = pick_chain_step(c, step);
            if (C.prev >= 0) {
                unsigned long long v[2] = {PS_LOW, PS_LOW};
                if (!ps_poll<2>(A.amin + (c * 64 + lane) * 2, 1, lane < end, v, ptag)) s_fail = 1;
                unsigned long long bv = v[0] & PS_LOW;
                int                bi = (v[1] & PS_LOW) == PS_LOW ? (1 << 30) : (int)(v[1] & PS_LOW);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long ov = __shfl_xor(bv, o);
                    const int                oi = __shfl_xor(bi, o);
                    if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
                }
                if (lane == 0) {
                    const bool any = bi < (1 << 30);
                    sl[c][C.prev]      = any ? bi >> 6 : 0;
                    sl[c][16 + C.prev] = any ? bi & 63 : 0;
                    if (C.shift)
                        for (int q = 0; q < C.nb - 1; q++) sl[c][q] = sl[c][q + 1], sl[c][16 + q] = sl[c][16 + q + 1];
                    if (li == 0 && C.nb_sel == PICK_FINISH) A.best[c] = any ? bv : ((uint64_t)1 << 63);
                }
            }
        }
        __syncthreads();
        if (li == 0 && t < MAX_CHAINS * 32 && pick_chain_step(t >> 5, step).nb_sel == PICK_FINISH) A.fin[t] = sl[t >> 5][t & 31];
        if (step == NSTEPS) break; // the last step only finishes the longest chain
        if (A.stat && t == 0) tk[2] += __builtin_amdgcn_s_memrealtime() - t0, t0 = __builtin_amdgcn_s_memrealtime();
        // 2. per-FB best over each live chain's selection (EbEncCdef.c:645-651): wave c, lane f
        {
            const int       c = w;
            const PickChainStep C = pick_chain_step(c, step);
            if (C.nb_sel >= 0 && lane < nfb) {
                uint64_t b = (uint64_t)1 << 63;
                for (int q = 0; q < C.nb_sel; q++) {
                    const int      j = sl[c][q], k = sl[c][16 + q];
                    const uint64_t v = wide ? m64[lane * 128 + j] + m64[lane * 128 + 64 + k]
                                            : (uint64_t)m32[lane * 128 + j] + m32[lane * 128 + 64 + k];
                    b = v < b ? v : b;
                }
                sb[c][lane] = b;
            }
        }
        __syncthreads();
        // 3. partial sums of rows 16 g + 4 w + {0..3}, column k = lane, of every live chain over the chunk
        const int j0 = 16 * g + 4 * w, k = lane;
#pragma unroll 1
        for (int c = 0; c < MAX_CHAINS; c++) {
            if (pick_chain_step(c, step).nb_sel < 0) continue;
            uint64_t acc[4] = {0, 0, 0, 0};
            if (!wide) {
#pragma unroll 4
                for (int f = 0; f < nfb; f++) {
                    const uint64_t b64 = sb[c][f];
                    const uint32_t b = b64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b64, m1k = m32[f * 128 + 64 + k];
                    const uint4    m0 = *(const uint4 *)&m32[f * 128 + j0];
                    acc[0] += min(m0.x + m1k, b), acc[1] += min(m0.y + m1k, b);
                    acc[2] += min(m0.z + m1k, b), acc[3] += min(m0.w + m1k, b);
                }
            } else {
#pragma unroll 1
                for (int f = 0; f < nfb; f++) {
                    const uint64_t b = sb[c][f], m1k = m64[f * 128 + 64 + k];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint64_t v = m64[f * 128 + j0 + u] + m1k;
                        acc[u] += v < b ? v : b;
                    }
                }
            }
            if (k < end)
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (j0 + u < end) ps_store(A.part + ((size_t)(ci * 4 + c) * 4096 + (j0 + u) * 64 + k), tag | acc[u]);
        }
        if (A.stat && t == 0) tk[0] += __builtin_amdgcn_s_memrealtime() - t0, t0 = __builtin_amdgcn_s_memrealtime();
        // 4. row owners: row j of the a-th live chain belongs to workgroup a * 64 + j (a < live chains, j < end)
        {
            int na = 0, c = -1;
            for (int q = 0; q < MAX_CHAINS; q++)
                if (pick_chain_step(q, step).nb_sel >= 0) {
                    if (na == (li >> 6)) c = q;
                    na++;
                }
            const int j = li & 63;
            if (c >= 0 && j < end) {
                unsigned long long s = 0;
                if (k < end && !ps_poll_sum<PS_NCH / 4>(A.part + (size_t)(w * 4 + c) * 4096 + j * 64 + k, (size_t)16 * 4096, tag, s))
                    s_fail = 1;
                red[t] = s;
                __syncthreads();
                if (w == 0) {
                    unsigned long long bv = PS_LOW;
                    int                bi = 1 << 30;
                    if (k < end) bv = red[k] + red[64 + k] + red[128 + k] + red[192 + k], bi = j * 64 + k;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long ov = __shfl_xor(bv, o);
                        const int                oi = __shfl_xor(bi, o);
                        if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
                    }
                    if (lane == 0) {
                        ps_store(A.amin + (c * 64 + j) * 2, tag | (bv & PS_LOW));
                        ps_store(A.amin + (c * 64 + j) * 2 + 1, tag | (unsigned long long)bi);
                    }
                }
            }
        }
        if (A.stat && t == 0) tk[1] += __builtin_amdgcn_s_memrealtime() - t0;
    }
    __syncthreads();
    if (t == 0 && s_fail) atomicOr(A.status, 1);
    if (A.stat && t == 0 && li == 0) A.stat[0] += tk[0], A.stat[1] += tk[1], A.stat[2] += tk[2], A.stat[3] += 1;
}

// ---- the settle check: the launch path's steps after T skipped when every chain has settled by then ----
// One lane per chain applies pick_settle_chain (cdef_pick_plan.h: the period argument and the index arithmetic) to the
// lists the steps up to T left and writes the final list and value of a chain that settled before it finished.
// out->settled = 1 when every unfinished chain settled, out->step = the latest step at which a chain that needs one
// settled (or finished): the host's next T.
// flag (device memory, asynchronous pick): the settled word the later steps read
// dep: the persistent fallback's epoch (asynchronous pick), raised when the check finds a chain unsettled -- only then
// does the fallback launch run, so its exchange words' epochs differ from those of its last four real runs
__global__ void pick_settle_kernel(const int32_t *lev, const uint64_t *val, int32_t *fin, uint64_t *best, int T,
                                   SettleOut *out, int32_t *flag, int seq, uint32_t *dep) {
    __shared__ int s_ok[MAX_CHAINS], s_at[MAX_CHAINS];
    const int c = threadIdx.x;
    if (c < MAX_CHAINS) {
        const PickSettle S = pick_settle_chain(lev, c, T);
        if (S.copies()) pick_settle_write(lev, val, c, S, fin, best);
        s_ok[c] = S.settled, s_at[c] = S.at;
    }
    __syncthreads();
    if (c == 0) {
        const int ok = s_ok[0] && s_ok[1] && s_ok[2] && s_ok[3];
        if (flag) *flag = ok;
        if (dep && !ok) *dep += 1;
        out->settled = ok;
        out->step    = max(max(s_at[0], s_at[1]), max(s_at[2], s_at[3]));
        if (seq) {
            __threadfence_system();
            __hip_atomic_store(&out->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- RD choice over the number of signalled strengths (EbEncCdef.c:853-872), per-FB strengths, parameters ----
// dprm: the asynchronous pick's frame parameters in device memory (what svtgpu_cdef_apply_frame reads with
// params == NULL), or null
__global__ void pick_final_kernel(const uint64_t *best, const int32_t *fin, const int32_t *count, uint64_t lambda,
                                  PickOut *out, int32_t *status, const uint64_t *wmse, const int32_t *fb_inv, int nfb,
                                  int8_t *fb_strength, int8_t *host_fbs, SvtGpuCdefParams *dprm, const PickMap map,
                                  int seq) {
    __shared__ int32_t gi[32];
    __shared__ int32_t s_nb;
    const int t = threadIdx.x;
    if (t == 0) { // every workgroup makes the same choice; workgroup 0 publishes it
        const int        sb_count = *count;
        const PickChoice ch       = pick_rd_choice(best, sb_count, lambda);
        pick_chosen_list(fin, ch, gi);
        s_nb = 1 << ch.nbits;
        if (blockIdx.x == 0) {
            for (int j = 0; j < 32; j++) out->gi[j] = gi[j];
            out->sb_count = sb_count;
            out->nbits    = ch.nbits;
            for (int c = 0; c < MAX_CHAINS; c++) out->best[c] = best[c];
            out->status = *status; // the persistent kernel's (0 on the launch path), re-armed for the next pick
            *status     = 0;
            if (dprm) *dprm = pick_params_from(map, ch.nbits, gi);
            if (seq) {
                __threadfence_system();
                __hip_atomic_store(&out->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    __syncthreads();
    // per-FB strength index (EbEncCdef.c:866-890), skipped FBs 0; also into the host's copy
    const int fb = blockIdx.x * blockDim.x + t;
    if (fb >= nfb) return;
    const int i  = fb_inv[fb];
    const int bg = i >= 0 ? pick_fb_strength(wmse + (size_t)i * 128, wmse + (size_t)i * 128 + 64, gi, s_nb) : 0;
    fb_strength[fb] = (int8_t)bg;
    if (host_fbs) host_fbs[fb] = (int8_t)bg;
}

// ---- the host path ----
// the pick's buffers of a state, carved by PickLayout
struct PickBufs {
    uint64_t           *wmse, *tot, *val, *best;
    uint32_t           *wmse32;
    int32_t            *lev, *fin, *wide, *fb_list, *count, *fb_inv;
    unsigned long long *part, *amin, *stat; // the persistent kernel's exchange and diagnostics
    int32_t            *status;
    int32_t            *flag; // the asynchronous pick: the settled word, the fallback's epoch, the apply's parameters
    uint32_t           *dep;
    SvtGpuCdefParams   *dprm;
    PickOut            *h_out, *d_out; // the mapped record: host and device addresses
    SettleOut          *h_settle, *d_settle;
    int8_t             *h_fbs, *d_fbs;
};
static PickBufs pick_bufs(const SvtGpuCdefFrameState *s) {
    const PickLayout L(s->nfb);
    PickBufs         B;
    B.wmse = s->d_pick_part + L.part_wmse, B.tot = s->d_pick_part + L.part_tot, B.val = s->d_pick_part + L.part_val;
    B.wmse32 = (uint32_t *)(s->d_pick_part + L.part_wmse32);
    B.best   = s->d_pick_out;
    B.lev = s->d_pick_lev + L.lev_lev, B.fin = s->d_pick_lev + L.lev_fin, B.wide = s->d_pick_lev + L.lev_wide;
    B.fb_list = s->d_fb_list + L.list_fb, B.count = s->d_fb_list + L.list_count, B.fb_inv = s->d_fb_list + L.list_inv;
    unsigned long long *xch = (unsigned long long *)s->d_pick_xch;
    B.part = xch + L.xch_part, B.amin = xch + L.xch_amin, B.stat = xch + L.xch_stat;
    B.status = (int32_t *)(xch + L.xch_status);
    uint8_t *ap = (uint8_t *)s->d_apick;
    B.flag = (int32_t *)(ap + L.apick_flag), B.dep = (uint32_t *)(ap + L.apick_dep);
    B.dprm = (SvtGpuCdefParams *)(ap + L.apick_params);
    B.h_out = (PickOut *)(s->h_pick + L.rec_out), B.d_out = (PickOut *)(s->h_pick_dev + L.rec_out);
    B.h_settle = (SettleOut *)(s->h_pick + L.rec_settle), B.d_settle = (SettleOut *)(s->h_pick_dev + L.rec_settle);
    B.h_fbs = (int8_t *)(s->h_pick + L.rec_fbs), B.d_fbs = (int8_t *)(s->h_pick_dev + L.rec_fbs);
    return B;
}

// the non-skipped FBs in raster order, then their rows with the zero-strength bias; tot0: the first step's accumulators
// to clear (launch path) or null
static void launch_compact_gather(const SvtGpuCdefFrameState *s, const PickBufs &B, int bias, uint64_t *tot0, hipStream_t st) {
    const int nfb = s->nfb;
    hipLaunchKernelGGL(pick_compact_kernel, dim3(1), dim3(NT), 0, st, s->d_skip, nfb, B.fb_list, B.count, B.wide, B.fb_inv);
    hipLaunchKernelGGL(pick_gather_kernel, dim3(nfb), dim3(128), 0, st, s->d_mse, nfb, B.fb_list, B.count, bias, B.wmse,
                       B.wmse32, B.wide, tot0);
}

// The persistent kernel's exchange words are valid by their tags alone, and words of a different strength count could
// carry a current tag: they are cleared, in stream order, when `end` changes.  Before every persistent launch.
static int xch_prepare(SvtGpuCdefFrameState *s, int end, hipStream_t st) {
    if (s->pick_xch_end == end) return SVTGPU_OK;
    HIP_TRY(hipMemsetAsync(s->d_pick_xch, 0, PickLayout::xch_bytes, st));
    s->pick_xch_end = end;
    return SVTGPU_OK;
}

// One persistent launch runs the whole pick.  The pick proper: tagged by the host's epoch, diagnostics in stat (or
// null).  The asynchronous pick's fallback: returns at once when *skip says every chain settled at the check, tagged by
// the epoch *dep the check counts on the device.
static void launch_persist(const PickBufs &B, int nfb, int end, uint32_t epoch, unsigned long long *stat,
                           const int32_t *skip, const uint32_t *dep, hipStream_t st) {
    PersistArgs P;
    P.wmse     = B.wmse;
    P.count    = B.count;
    P.wide     = B.wide;
    P.chunk    = ps_chunk(nfb);
    P.fb_alloc = nfb;
    P.end_gi   = end;
    P.epoch    = epoch;
    P.part     = B.part;
    P.amin     = B.amin;
    P.fin      = B.fin;
    P.best     = B.best;
    P.status   = B.status;
    P.stat     = stat;
    P.skip     = skip;
    P.dep      = dep;
    hipLaunchKernelGGL(sod_persist_kernel, dim3(PS_GRID), dim3(NT), 0, st, P);
}

// what every step launch of a pick shares
static StepArgs step_args(const PickBufs &B, int nfb, int end) {
    StepArgs A{};
    A.wmse = B.wmse, A.wmse32 = B.wmse32, A.count = B.count, A.wide = B.wide;
    A.start_gi = 0, A.end_gi = end, A.fb_alloc = nfb;
    A.tot = B.tot, A.lev = B.lev, A.fin = B.fin, A.best = B.best, A.val = B.val;
    return A;
}
// step `step` of the launch path: the schedule's entry of every chain that has not ended, shaped for their number.
// skip: the asynchronous pick's settled word (steps after the check) or null
static void launch_step(StepArgs &A, int step, const PickKnobs &K, const int32_t *skip, hipStream_t st) {
    int na = 0;
    for (int c = 0; c < MAX_CHAINS; c++) {
        const PickChainStep C = pick_chain_step(c, step);
        if (C.nb_sel != PICK_ENDED) A.ch[na++] = StepChain{c, C.nb, C.nb_sel, C.prev, C.shift};
    }
    const PickStepShape sh = pick_step_shape(K, A.fb_alloc, na);
    A.step = step, A.na = na, A.chunk = sh.chunk, A.skip = skip;
    A.wgclk = svtgpu_wgclk_begin(sh.grid);
    hipLaunchKernelGGL(sod_step_kernel, dim3(sh.grid), dim3(NT), sh.lds, st, A);
    svtgpu_wgclk_end("sod_step", sh.grid, st);
}

// The settle check after step T, in stream order.  The synchronous pick waits for its record; the asynchronous pick's
// later launches read its flag instead, its record carries a sequence number for the host to take later, and with a
// persistent fallback (pfb) the check counts that launch's epoch.
static int launch_settle(SvtGpuCdefFrameState *s, const PickBufs &B, int T, bool async_, bool pfb, hipStream_t st) {
    hipLaunchKernelGGL(pick_settle_kernel, dim3(1), dim3(64), 0, st, (const int32_t *)B.lev, (const uint64_t *)B.val,
                       B.fin, B.best, T, B.d_settle, async_ ? B.flag : (int32_t *)nullptr, async_ ? ++s->settle_seq : 0,
                       pfb ? B.dep : (uint32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

// The launch path: steps 0 .. NSTEPS with the settle check after step T (T == NSTEPS: no check).  Synchronous: the
// host waits for the check and stops launching when every chain has settled (one wait instead of up to 40 - T
// dependent launches, each of which waits for free CU slots when other frames' kernels hold the device).
// Asynchronous: no wait -- with the persistent fallback (pfb) no step follows the check; else the later steps read
// the check's flag and return at once when every chain has settled.
static int run_steps(SvtGpuCdefFrameState *s, const PickBufs &B, const PickKnobs &K, int end, int T, bool async_, bool pfb,
                     hipStream_t st) {
    StepArgs  A    = step_args(B, s->nfb, end);
    const int last = pfb ? T : NSTEPS;
    for (int step = 0; step <= last; step++) {
        launch_step(A, step, K, async_ && step > T ? B.flag : nullptr, st);
        if (step != T || T == NSTEPS) continue;
        if (int rc = launch_settle(s, B, T, async_, pfb, st)) return rc;
        if (async_) continue;
        if (int rc = svtgpu_comm_wait(s->comm, st)) return rc; // bounded behind the tables' exchange
        svtgpu_count_xfer(1, sizeof(SettleOut));
        s->pick_policy.outcome_sync(B.h_settle->settled != 0, B.h_settle->step, T);
        if (B.h_settle->settled) break;
    }
    return SVTGPU_OK;
}

// The asynchronous pick learns a check's outcome from the last record that has landed, read without a wait (the host may
// run ahead of the device), at the start of a later pick.
static void settle_take_async(SvtGpuCdefFrameState *s, const PickBufs &B) {
    const volatile SettleOut *hs = B.h_settle;
    if (hs->seq == 0 || hs->seq == s->settle_seen) return;
    s->settle_seen = hs->seq;
    s->pick_policy.outcome_async(hs->settled != 0, hs->step);
}

// the pick's result from the mapped record (after the stream wait): the parameters through the strength map, the
// per-FB strengths
static void cdef_pick_host_result(SvtGpuCdefFrameState *s, const PickMap &map, SvtGpuCdefParams *params,
                                  int8_t *fb_strength_out) {
    const PickBufs B = pick_bufs(s);
    *params          = pick_params_from(map, B.h_out->nbits, B.h_out->gi);
    if (fb_strength_out) memcpy(fb_strength_out, B.h_fbs, s->nfb);
    svtgpu_count_xfer(1, sizeof(PickOut) + (fb_strength_out ? s->nfb : 0)); // mapped memory
}

// the synchronous pick's only wait (bounded when tiled), then its result; stat: the persistent kernel's diagnostics or null
static int pick_read_sync(SvtGpuCdefFrameState *s, const PickBufs &B, unsigned long long *stat, const PickMap &map,
                          SvtGpuCdefParams *params, int8_t *fb_strength_out, hipStream_t st) {
    if (int rc = svtgpu_comm_wait(s->comm, st)) return rc;
    if (B.h_out->status) {
        svtgpu_set_last_hip_error(hipErrorUnknown, "CDEF pick: the persistent step exchange timed out", __FILE__, __LINE__);
        return SVTGPU_ERR_HIP;
    }
    if (stat) {
        unsigned long long v[4];
        HIP_TRY(hipMemcpy(v, stat, sizeof v, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(stat, 0, sizeof v));
        std::fprintf(stderr, "sod_persist (workgroup 0): compute+store %.1f us, reduce %.1f us, minima %.1f us\n",
                     v[0] * 0.01, v[1] * 0.01, v[2] * 0.01);
    }
    cdef_pick_host_result(s, map, params, fb_strength_out);
    return SVTGPU_OK;
}

// params == nullptr: the asynchronous pick (svtgpu_cdef_pick_async) -- no host wait: the settle check's outcome reaches
// the later steps through a device flag (they exit at once when every chain has settled), the final kernel writes the
// frame parameters to device memory for the apply, and the host reads the result later (svtgpu_cdef_read_params).
// After the check the asynchronous pick launches no further step: when a chain has not settled, one persistent launch
// (which returns at once when the check's flag says settled) recomputes the whole pick.  The flag-only step launches it
// replaces each needed 256 workgroup slots, which at four frames in flight waited for CUs held by other frames'
// kernels.  Frames with more FBs than its chunks hold, and SVTGPU_PICK_ASYNC_FALLBACK=steps, keep the flagged launches.
int svtgpu_cdef_pick_impl(SvtGpuCdefFrameState *s, const SvtGpuCdefControls *ctrls, int32_t base_q_idx,
                          uint64_t lambda, SvtGpuCdefParams *params, int8_t *fb_strength_out, hipStream_t st) {
    const bool async_ = params == nullptr;
    const int  nfb = s->nfb, end = ctrls->first_pass_fs_num + ctrls->default_second_pass_fs_num;
    if (end <= 0 || end > 64)
        return SVTGPU_ERR_INVALID_ARG;
    const PickKnobs K       = pick_knobs();
    const PickBufs  B       = pick_bufs(s);
    const bool      persist = K.persist && ps_fits(nfb); // while its chunks hold every FB
    launch_compact_gather(s, B, ctrls->zero_fs_cost_bias, persist ? nullptr : B.tot, st);
    if (async_) settle_take_async(s, B);
    const int  T   = s->pick_policy.begin(K.settle); // on either path: a persistent pick counts as one without a check
    const bool pfb = async_ && !persist && !K.async_steps && T < NSTEPS && ps_fits(nfb); // the persistent fallback
    unsigned long long *stat = persist && K.stats ? B.stat : nullptr;
    if (persist || pfb)
        if (int rc = xch_prepare(s, end, st)) return rc;
    if (persist) launch_persist(B, nfb, end, s->pick_epoch++, stat, nullptr, nullptr, st);
    else if (int rc = run_steps(s, B, K, end, T, async_, pfb, st)) return rc;
    if (pfb) launch_persist(B, nfb, end, 0, nullptr, B.flag, B.dep, st);
    HIP_TRY(hipGetLastError());
    const PickMap map = pick_map_from(*ctrls, base_q_idx);
    hipLaunchKernelGGL(pick_final_kernel, dim3((nfb + NT - 1) / NT), dim3(NT), 0, st, (const uint64_t *)B.best,
                       (const int32_t *)B.fin, (const int32_t *)B.count, lambda, B.d_out, B.status, (const uint64_t *)B.wmse,
                       (const int32_t *)B.fb_inv, nfb, s->d_fb_strength, fb_strength_out || async_ ? B.d_fbs : (int8_t *)nullptr,
                       async_ ? B.dprm : (SvtGpuCdefParams *)nullptr, map, async_ ? ++s->apick_seq : 0);
    HIP_TRY(hipGetLastError());
    if (!async_) return pick_read_sync(s, B, stat, map, params, fb_strength_out, st);
    std::memcpy(s->apick_map, map.code, 64); // the read-back's strength map
    s->apick_damping = map.damping;
    return SVTGPU_OK;
}

// svtgpu_cdef_read_params: the last asynchronous pick's result, after a (bounded) wait for the stream
int svtgpu_cdef_pick_read(SvtGpuCdefFrameState *s, SvtGpuCdefParams *params, int8_t *fb_strength_out, hipStream_t st) {
    if (int rc = svtgpu_comm_wait(s->comm, st)) return rc;
    s->apick_pending = 0;
    if (s->apick_ref) { // the reference-fs parameters (no search): known when the pick was enqueued
        *params = s->apick_params;
        if (fb_strength_out) memset(fb_strength_out, 0, s->nfb);
        return SVTGPU_OK;
    }
    const volatile PickOut *h_out = pick_bufs(s).h_out;
    if (h_out->seq != s->apick_seq) {
        svtgpu_set_last_hip_error(hipErrorUnknown, "CDEF asynchronous pick: result record missing after the stream wait",
                                  __FILE__, __LINE__);
        return SVTGPU_ERR_HIP;
    }
    if (h_out->status) {
        svtgpu_set_last_hip_error(hipErrorUnknown, "CDEF pick: the persistent step exchange timed out", __FILE__, __LINE__);
        return SVTGPU_ERR_HIP;
    }
    PickMap map;
    std::memcpy(map.code, s->apick_map, 64);
    map.damping = s->apick_damping;
    cdef_pick_host_result(s, map, params, fb_strength_out);
    return SVTGPU_OK;
}
