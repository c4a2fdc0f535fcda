"""The temporal filter's sub-pel search (svtgpu_tf_search_frame) and the whole device chain behind it
(svtgpu_tf_compensate_filter_frame) on the MI355X, timed with HIP events after warm-up.

Workloads (synthetic, stated): a 1920x1080 8-bit and a 3840x2160 10-bit 4:2:0 picture and 6 padded reference pictures
(border 80).  The centre is 4x4-blocky noise plus fine noise; reference r is the centre moved by a whole number of samples
that changes per 96x96 region, plus noise whose strength changes per region (0, 2, 6 or 20 grey levels at 8 bits), so that the
walk ends on all of its paths; the full-pel MVs are the region's motion, off by one sample in a quarter of the draws.
Default search parameters (all modes 1, 8x8 on, thresholds 0, no sub-sampling).  The full-pel upload (352 bytes per
reference and block) is part of the timed search call.  Best of 3 x `reps` calls.

    python3 scripts/tf_search_perf.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "svt-av1_pro-anchor-v2.1.0-_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svtgpu  # noqa: E402

SHAPES = [(8, 1920, 1080), (10, 3840, 2160)]
N_REFS = 6
PAD = 80


def timed(stream, reps, fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(stream):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime takes the device before libsvtgpu's
    ctx = svtgpu.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    L = svtgpu.lib()
    for bd, w, h in SHAPES:
        rng = np.random.default_rng(0x5453 + bd)
        aw, ah, dt, sc = (w + 63) & ~63, (h + 63) & ~63, np.uint16 if bd > 8 else np.uint8, 1 << (bd - 8)
        bs, maxv = (2 if bd > 8 else 1), (1 << bd) - 1
        st = svtgpu.TfState(ctx, w, h)
        big_h, big_w = ah + 2 * PAD + 32, aw + 2 * PAD + 32  # the texture, with room for the motion
        tex = np.repeat(np.repeat(rng.integers(0, 160 * sc, (big_h // 4 + 1, big_w // 4 + 1)), 4, 0), 4, 1)[:big_h, :big_w]
        tex = tex + rng.integers(0, 24 * sc, tex.shape)
        cen = [tex[PAD + 16:PAD + 16 + ah, PAD + 16:PAD + 16 + aw].astype(dt)]
        cen += [rng.integers(0, maxv + 1, (ah // 2, aw // 2)).astype(dt) for _ in range(2)]
        ry, rx = np.mgrid[0:h + 2 * PAD, 0:w + 2 * PAD]
        region = (ry // 96) * ((w + 2 * PAD) // 96 + 1) + rx // 96
        refs, fullpel = [], []
        for r in range(N_REFS):
            nreg = int(region.max()) + 1
            mx, my, amp = rng.integers(-3, 4, nreg), rng.integers(-3, 4, nreg), np.array([0, 2, 6, 20])[rng.integers(0, 4, nreg)] * sc
            y = tex[ry + 16 + my[region], rx + 16 + mx[region]] + rng.integers(-1, 2, region.shape) * amp[region]
            refs.append([np.clip(y, 0, maxv).astype(dt)] +
                        [rng.integers(0, maxv + 1, ((h + 2 * PAD) // 2, (w + 2 * PAD) // 2)).astype(dt) for _ in range(2)])
            for blk in range(st.nblk):
                bx, by = (blk % (aw // 64)) * 64, (blk // (aw // 64)) * 64

                jit, n = rng.integers(0, 8, (85, 2)), [0]

                def mv(x, y, s):  # the prediction reads the reference at x + mv: minus the content's motion
                    g = region[min(by + y + s // 2 + PAD, h + 2 * PAD - 1), min(bx + x + s // 2 + PAD, w + 2 * PAD - 1)]
                    j = jit[n[0]]
                    n[0] += 1
                    return (-int(mx[g]) + (j[0] == 0) - (j[0] == 1), -int(my[g]) + (j[1] == 0) - (j[1] == 1))
                m32 = [mv((i & 1) * 32, (i >> 1) * 32, 32) for i in range(4)]
                m16 = [mv((i & 1) * 32 + (j & 1) * 16, (i >> 1) * 32 + (j >> 1) * 16, 16) for i in range(4) for j in range(4)]
                m8 = [mv((i & 1) * 32 + (j & 1) * 16 + (k & 1) * 8, (i >> 1) * 32 + (j >> 1) * 16 + (k >> 1) * 8, 8)
                      for i in range(4) for j in range(4) for k in range(4)]
                fullpel.append(svtgpu.TfFullpel.make(mv(0, 0, 64), m32, m16, m8, 0))
        fa = (svtgpu.TfFullpel * len(fullpel))(*fullpel)
        dc, do = [dev(a) for a in cen], [dev(np.zeros(a.shape, dt)) for a in cen]
        dr = [[dev(a) for a in ref] for ref in refs]
        dp = [[dev(np.zeros((ah >> (p > 0), aw >> (p > 0)), dt)) for p in range(3)] for _ in range(N_REFS)]
        strides = [aw, aw >> 1, aw >> 1]
        cp, op = svtgpu.TfPlanes.make([t.data_ptr() for t in dc], strides), svtgpu.TfPlanes.make([t.data_ptr() for t in do], strides)
        pr = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make(
            [t[p].data_ptr() + (PAD >> (p > 0)) * (a[p].shape[1] + 1) * bs for p in range(3)], [a[p].shape[1] for p in range(3)])
            for t, a in zip(dr, refs)])
        pp = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make([t.data_ptr() for t in d], strides) for d in dp])
        sp = svtgpu.TfSearchParams.make((1, 1, 1), 0, 0, 1, 0, 0, bd)
        fprm = svtgpu.TfParams.make((6000000, 9000000, 12000000), 1080, 1, bd, 0)

        def search():
            svtgpu.check(L.svtgpu_tf_search_frame(st.h, cp, pr, N_REFS, PAD, PAD, fa, sp, None))

        def chain():
            search()
            svtgpu.check(L.svtgpu_tf_compensate_filter_frame(st.h, cp, pr, N_REFS, PAD, PAD, fprm, 0, pp, op, None))
        for _ in range(args.warmup):
            chain()
        ctx.synchronize()
        ms_s = [timed(stream, args.reps, search) for _ in range(3)]
        ms_c = [timed(stream, args.reps, chain) for _ in range(3)]
        mo, bl = st.search_read(N_REFS)
        n64 = sum(m.use64 for m in mo)
        n32 = sum(1 for m in mo if not m.use64 for i in range(4) if not m.split32[i])
        n16 = sum(1 for m in mo for q in range(16) if m.split32[q >> 2] and not m.split16[q])
        n8 = sum(4 for m in mo for q in range(16) if m.split32[q >> 2] and m.split16[q])
        out = [t.cpu().numpy().view(dt) for t in do]
        print(json.dumps({
            "metric": "tf_search_ms", "workload": "%dx%d %d-bit 4:2:0, %d references" % (w, h, bd, N_REFS), "reps": args.reps,
            "search_ms": [round(v, 4) for v in ms_s], "chain_ms": [round(v, 4) for v in ms_c],
            "search_us_per_ref_block": round(min(ms_s) * 1e3 / (N_REFS * st.nblk), 3),
            "blocks_64_32_16_8": [int(n64), n32, n16, n8], "sample_sum": int(sum(int(a.reshape(-1)[::97].sum()) for a in out)),
            "data": "synthetic"}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
