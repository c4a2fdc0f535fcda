"""Tie, boundary and large-frame tables for the frame-level CDEF strength pick, and a plain restatement of it.

Shared by test_cdef_pick_ties.py (CPU: the oracle's pick against the restatement below, and the "reach" assertions
that a table really ties or sits on the boundary it is built for) and test_cdef_pick_ties_gpu.py (the device's pick
against the oracle, bit for bit).  Every case is built once (lru_cache) and its arrays are read-only.

The restatement follows finish_cdef_search, joint_strength_search_dual and svt_search_one_dual_c of the reference
(EbEncCdef.c:627-926) line by line in numpy uint64 / Python ints; it shares no code with oracle/cdef_oracle.c or
with the device's pick.

A case is the tuple (family, arg, width, height, cdef level, lambda, skip pattern).  Families, with j = arange(64)
the strength index (mse[0] luma, mse[1] chroma, one row per 64x64 filter block):
  const     every entry arg: every strength pair of every svt_search_one_dual call ties
  one_wide  const 1000 with the single entry mse[arg[0]][last live FB][arg[1]] = 2^31
  mod       1000 * ((j + 3) % 4) + 500 luma, 700 * ((j + 5) % 8) + 100 chroma: periodic ties, first minimum not at 0
  lane      65536 * (j not in {5, 8}) + 9 luma, 65536 * (j not in {3, 8}) + 9 chroma: the four minimal pairs are
            e = 64 j + k = 323, 328, 515, 520
  two       FBs alternate between two populations with different optima
  four      FBs cycle through four populations
  tie3      two's populations and a third whose rows are constant: its blocks cost the same under every signalled
            strength and must take index 0
  wide_lane 2^31 - 10 * (j in {5, 8}) luma, 2^31 chroma: the minimal sums are 2^32 - 10, every other is 2^32
  noise     random entries just below 2^31 with a random strength-0 entry: practically no ties (the control)
Skip patterns: ("none",), ("last", n): only the last n FBs of the frame are live, ("only", i): FB i (negative: from
the end) alone is live, ("rand",): each FB skipped with probability 0.1."""
import functools

import numpy as np

import oracle

Q = 128          # base_q_idx of every case (it only sets the damping)
LAMBDA = 60000   # the lambda of the other pick tests
W31 = 1 << 31    # pick_gather_kernel's width limit: an entry >= 2^31 selects the 64-bit accumulation
TOP = 1 << 63    # best_tot_mse / best_mse initial value (EbEncCdef.c:631, 639, 736, 880)
M64 = (1 << 64) - 1
D_LANE, D_POP = 1 << 16, 1 << 20
J = np.arange(64, dtype=np.int64)


def nfb_of(w, h):
    return ((h // 4 + 15) // 16) * ((w // 4 + 15) // 16)


def family_rows(family, arg, r=0):
    """(luma row, chroma row) of population r of a family, int64 [64] each."""
    if family == "const":
        return np.full(64, arg, np.int64), np.full(64, arg, np.int64)
    if family == "mod":
        return 1000 * ((J + 3) % 4) + 500, 700 * ((J + 5) % 8) + 100
    if family == "lane":
        return D_LANE * ~np.isin(J, (5, 8)) + 9, D_LANE * ~np.isin(J, (3, 8)) + 9
    if family == "two":
        return D_POP * ((J + 1 + r) % 4) + 64, D_POP * ((J + (2, 7)[r]) % 8) + 64
    if family == "four":
        return D_POP * ((J + r + 1) % 5) + 64, D_POP * ((J + 3 * r + 2) % 7) + 64
    if family == "tie3":
        return family_rows("two", arg, r) if r < 2 else (np.full(64, D_POP, np.int64), np.full(64, D_POP, np.int64))
    if family == "wide_lane":
        return W31 - 10 * np.isin(J, (5, 8)), np.full(64, W31, np.int64)
    raise KeyError(family)


POPULATIONS = {"const": 1, "mod": 1, "lane": 1, "two": 2, "four": 4, "tie3": 3, "wide_lane": 1}


def skip_of(pattern, nfb, rng=None):
    skip = np.ones(nfb, np.uint8)
    if pattern[0] == "none":
        skip[:] = 0
    elif pattern[0] == "last":
        skip[nfb - pattern[1]:] = 0
    elif pattern[0] == "only":
        skip[pattern[1]] = 0
    elif pattern[0] == "rand":
        skip = (rng.random(nfb) < 0.1).astype(np.uint8)
    else:
        raise KeyError(pattern)
    return skip


def tables(family, arg, w, h, pattern):
    """(mse uint64 [2][nfb][64], skip uint8 [nfb])"""
    nfb = nfb_of(w, h)
    rng = np.random.default_rng(1000003 * w + h)
    if family == "noise":  # test_cdef_pick_bound_tables_vs_oracle's construction at top = 2^31
        mse = (W31 - 1 - rng.integers(0, W31 // 64, size=(2, nfb, 64), dtype=np.int64)).astype(np.uint64)
        mse[:, :, 0] = rng.integers(0, W31 // 2, size=(2, nfb)).astype(np.uint64)
        return mse, skip_of(pattern, nfb, rng)
    skip = skip_of(pattern, nfb, rng)
    mse = np.zeros((2, nfb, 64), np.uint64)
    if family == "one_wide":
        mse[:] = 1000
        mse[arg[0], np.nonzero(skip == 0)[0][-1], arg[1]] = W31
        return mse, skip
    npop = POPULATIONS[family]
    for r in range(npop):
        m0, m1 = family_rows(family, arg, r)
        mse[0, r::npop], mse[1, r::npop] = m0.astype(np.uint64), m1.astype(np.uint64)
    return mse, skip


class Case:
    def __init__(self, key):
        self.key = key
        self.family, self.arg, self.w, self.h, self.level, self.lam, self.pattern = key
        self.nfb = nfb_of(self.w, self.h)
        self.mse, self.skip = tables(self.family, self.arg, self.w, self.h, self.pattern)
        self.mse.setflags(write=False)
        self.skip.setflags(write=False)
        self.live = int((self.skip == 0).sum())

    @functools.lru_cache(maxsize=None)
    def want(self, level=None):
        """The oracle's pick at the case's level (or another): (parameter tuple, per-FB strength indices)."""
        level = self.level if level is None else level
        prm, fbs = oracle.cdef_pick(self.w, self.h, self.mse, self.skip, oracle.controls(level), Q, self.lam)
        fbs.setflags(write=False)
        return prm.as_tuple(), fbs

    @functools.lru_cache(maxsize=None)
    def restated(self):
        """((parameter tuple, per-FB strength indices), trace) of the restatement at the case's level."""
        trace = []
        res = finish_cdef_search(self.mse, self.skip, oracle.controls(self.level), Q, self.lam, trace)
        res[1].setflags(write=False)
        return res, trace


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


def case_id(key):
    family, arg, w, h, level, lam, pattern = key
    a = "" if arg is None else "-".join(str(x) for x in (arg if isinstance(arg, tuple) else (arg,)))
    return "%s%s_%dx%d_l%d_lam%d_%s" % (family, a, w, h, level, lam, "".join(str(x) for x in pattern))


def K(family, w, h, arg=None, level=1, lam=None, pattern=("none",)):
    if family == "const" and arg is None:
        arg = 1000
    if lam is None:
        lam = 1 if family == "four" else LAMBDA  # four: a small lambda lets the RD choice signal four strengths
    return (family, arg, w, h, level, lam, pattern)


NONE = ("none",)
# 1, 2, 3, 5 FBs: fewer than a step's smallest chunk of 4, partial last chunks; 65: one more than a 64-lane wave
TINY = [K(f, w, 64) for w in (64, 128, 192, 320, 4160) for f in ("const", "lane", "two", "four")]
# 1920x1080 (510 FBs): with four chains live a step's chunk is 32 FBs, with one chain 8; the live FBs are the frame's
# last, behind more than 256 skipped ones (pick_compact_kernel's second 256-thread round)
CHUNK_LIVE = (32, 33, 8, 9)
CHUNK = [K(f, 1920, 1080, pattern=("last", n)) for n in CHUNK_LIVE for f in ("const", "lane", "four", "noise")] + \
        [K("two", 1920, 1080, pattern=("last", 32))]
SINGLE = [K(f, 1920, 1080, pattern=("only", i)) for i in (0, -1) for f in ("mod", "lane")]
FULL_1080 = [K(f, 1920, 1080) for f in ("const", "lane", "two", "four")] + [K("noise", 1920, 1080, pattern=("rand",))]
# 2040 FBs: the persistent kernel's 64 chunks of 32 nearly full; the three widths of const
UHD = [K("const", 3840, 2160, arg=v) for v in (1000, W31 - 1, W31)] + [K("four", 3840, 2160)]
# above the persistent kernel's 2048 FBs: 2304 and 8160
LARGE = [k for (w, h) in ((4096, 2304), (7680, 4320))
         for k in (K("four", w, h), K("two", w, h, pattern=("last", 33)), K("noise", w, h, pattern=("rand",)))]
LEVELS = [K(f, 256, 192, level=lv) for lv in (1, 2, 5, 9, 12) for f in ("const", "mod", "two")]
# the width flag: const at the narrow limit and above it, the zero-strength bias of level 12 (62/64) bringing entry 0
# back under 2^31, and one wide entry among narrow ones -- at strength 0, and at strength 63 of the chroma row at a
# level that searches 48 strengths (the flag is raised by an entry no call reads)
WIDE = [K("const", 1024, 512, arg=W31 - 1), K("const", 1024, 512, arg=W31), K("const", 1024, 512, arg=W31, level=12),
        K("one_wide", 1024, 512, arg=(0, 0)), K("one_wide", 1024, 512, arg=(1, 63), level=2),
        K("one_wide", 1920, 1080, arg=(0, 0), pattern=("last", 33))]
LAMBDA0 = [K("const", 256, 192, lam=0), K("two", 256, 192, lam=0)]
# blocks that tie between the signalled strengths (the per-FB assignment's first minimum); sums on either side of 2^32
FB_TIES = [K("tie3", 320, 64), K("tie3", 1920, 1080), K("tie3", 1920, 1080, pattern=("last", 33)),
           K("tie3", 4096, 2304), K("wide_lane", 1024, 512), K("wide_lane", 256, 192, level=2)]

ALL = TINY + CHUNK + SINGLE + FULL_1080 + UHD + LARGE + LEVELS + WIDE + LAMBDA0 + FB_TIES
assert len(set(ALL)) == len(ALL)
# the restatement is slow: frames up to 510 FBs, and one of 2040
RESTATED = [k for k in ALL if nfb_of(k[2], k[3]) <= 510] + [K("four", 3840, 2160)]


# ------------------------------------------------------------------------------------------ the restatement
def search_one_dual(lev0, lev1, nb_strengths, m0, m1, start_gi, end_gi, trace=None):
    """svt_search_one_dual_c (EbEncCdef.c:627-683).  m0, m1: uint64 [sb_count][64]."""
    sb_count = m0.shape[0]
    best_mse = np.full(sb_count, TOP, np.uint64)
    for gi in range(nb_strengths):                       # :644-649, strict <
        curr = m0[:, lev0[gi]] + m1[:, lev1[gi]]
        best_mse = np.where(curr < best_mse, curr, best_mse)
    tot_mse = np.zeros((64, 64), np.uint64)              # :635
    s = slice(start_gi, end_gi)
    for i0 in range(0, sb_count, 128):                   # :655-665, 128 filter blocks at a time
        i = slice(i0, i0 + 128)
        curr = m0[i, s, None] + m1[i, None, s]
        tot_mse[s, s] += np.minimum(curr, best_mse[i, None, None]).sum(axis=0, dtype=np.uint64)
    best_tot_mse, best_id0, best_id1 = TOP, 0, 0
    sub = tot_mse[s, s]
    if sub.size and int(sub.min()) < best_tot_mse:       # :670-679: the first minimum in (j, k) order
        e = int(np.argmin(sub))                          # numpy: the first occurrence in row-major order
        best_tot_mse = int(sub.min())
        best_id0, best_id1 = start_gi + e // sub.shape[1], start_gi + e % sub.shape[1]
    lev0[nb_strengths], lev1[nb_strengths] = best_id0, best_id1
    if trace is not None:
        trace.append({"nb_sel": nb_strengths, "start": start_gi, "end": end_gi, "tot": tot_mse, "best": best_tot_mse,
                      "pick": (best_id0, best_id1)})
    return best_tot_mse


def joint_strength_search_dual(best_lev0, best_lev1, nb_strengths, m0, m1, start_gi, end_gi, trace=None):
    """EbEncCdef.c:697-727"""
    best_tot_mse = TOP
    for i in range(nb_strengths):
        best_tot_mse = search_one_dual(best_lev0, best_lev1, i, m0, m1, start_gi, end_gi, trace)
    for i in range(4 * nb_strengths):
        for j in range(nb_strengths - 1):
            best_lev0[j], best_lev1[j] = best_lev0[j + 1], best_lev1[j + 1]
        best_tot_mse = search_one_dual(best_lev0, best_lev1, nb_strengths - 1, m0, m1, start_gi, end_gi, trace)
    return best_tot_mse


def rdcost(lam, rate, dist):
    """RDCOST(RM, R, D) = ROUND_POWER_OF_TWO((int64)R * (int64)RM, 9) + (int64)D * (1 << 7), stored in a uint64
    (EbRateDistortionCost.h:37-39): two's-complement arithmetic modulo 2^64."""
    return ((((rate * lam) + 256) >> 9) + dist * 128) & M64


def finish_cdef_search(mse, skip, ctrls, base_q_idx, lam, trace=None):
    """finish_cdef_search (EbEncCdef.c:796-921, use_reference_cdef_fs == 0, 64x64 superblocks): returns
    ((damping, bits, y strengths, uv strengths), per-FB strength index int8 [nfb] with skipped FBs at 0)."""
    nfb = len(skip)
    first, second = ctrls.first_pass_fs_num, ctrls.default_second_pass_fs_num
    start_gi, end_gi = 0, first + second
    sb_addr = [fb for fb in range(nfb) if not skip[fb]]                  # :819-840
    m0, m1 = np.array(mse[0][sb_addr], np.uint64), np.array(mse[1][sb_addr], np.uint64)
    sb_count = len(sb_addr)
    if ctrls.zero_fs_cost_bias:                                          # :845-851
        factor = np.uint64(ctrls.zero_fs_cost_bias)
        m0[:, 0] = (factor * m0[:, 0]) >> np.uint64(6)
        m1[:, 0] = (factor * m1[:, 0]) >> np.uint64(6)
    best_tot_mse, nb_strength_bits, y, uv = TOP, 0, [0] * 8, [0] * 8
    for i in range(4):                                                   # :853-872
        best_lev0, best_lev1 = [0] * 8, [0] * 8
        nb_strengths = 1 << i
        if trace is not None:
            trace.append({"chain": i})
        tot_mse = joint_strength_search_dual(best_lev0, best_lev1, nb_strengths, m0, m1, start_gi, end_gi, trace)
        total_bits = sb_count * i + nb_strengths * 6 * 2                 # CDEF_STRENGTH_BITS = 6
        rate_cost = total_bits * (1 << 9)                                # av1_cost_literal
        dist = (tot_mse * 16) & M64
        tot_mse = rdcost(lam, rate_cost, dist)
        if trace is not None:
            trace.append({"cost": tot_mse})
        if tot_mse < best_tot_mse:
            best_tot_mse, nb_strength_bits = tot_mse, i
            y[:nb_strengths], uv[:nb_strengths] = best_lev0[:nb_strengths], best_lev1[:nb_strengths]
    nb_strengths = 1 << nb_strength_bits
    fbs = np.zeros(nfb, np.int8)
    for i in range(sb_count):                                            # :877-892
        best_gi, best_mse = 0, TOP
        for gi in range(nb_strengths):
            curr = int(m0[i, y[gi]]) + int(m1[i, uv[gi]])
            if curr < best_mse:
                best_gi, best_mse = gi, curr
        fbs[sb_addr[i]] = best_gi
    filter_map = [0] * 64                                                # :911-919
    for i in range(first):
        filter_map[i] = ctrls.default_first_pass_fs[i]
    for i in range(first, first + second):
        filter_map[i] = ctrls.default_second_pass_fs[i - first]
    ys = tuple(filter_map[v] for v in y[:nb_strengths])
    uvs = tuple(filter_map[v] for v in uv[:nb_strengths])
    return (3 + (base_q_idx >> 6), nb_strength_bits, ys, uvs), fbs       # :921


def minimal_pairs(call):
    """The strength pairs e = 64 j + k of one traced svt_search_one_dual call whose total equals the minimum."""
    s = slice(call["start"], call["end"])
    tot = call["tot"]
    jj, kk = np.nonzero(tot[s, s] == tot[s, s].min())
    return [64 * (call["start"] + int(j)) + call["start"] + int(k) for j, k in zip(jj, kk)]
