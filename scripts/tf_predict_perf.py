"""The temporal filter's motion compensation (svtgpu_tf_predict_frame) on the MI355X, timed with HIP events after warm-up.

Workloads (synthetic, stated): a 1920x1080 8-bit and a 3840x2160 10-bit 4:2:0 picture, 6 padded reference pictures (border
80), a mixed partition (a quarter of the 64x64 blocks whole, else random 32 / 16 / 8 splits) and MVs that are zero, small
or far outside the picture.  Reported as a fraction of the HBM bandwidth from the algorithmic bytes: every reference picture
read once, every predictor picture written once (the 64-aligned area), the metadata once; the metadata upload (368 bytes
per reference and block) is part of the timed call.  Best of 3 x `reps` calls.
tests/golden/gen_golden_interp.c --time runs the same shapes, reference count and partition distribution (its own draw of
partitions and MVs) through the reference's C and AVX2 on one host core.

    python3 scripts/tf_predict_perf.py [--reps 50] [--warmup 10]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "svt-av1_pro-anchor-v2.1.0-_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import interp_cases as ic  # noqa: E402
import svtgpu  # noqa: E402

SHAPES = [(8, 1920, 1080), (10, 3840, 2160)]
N_REFS = 6
PAD = 80
HBM_PEAK = 8.0e12      # bytes/s, the MI355X's specified HBM3E bandwidth


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
    for bd, w, h in SHAPES:
        r = np.random.default_rng(0x4950 + bd)
        aw, ah, dt = (w + 63) & ~63, (h + 63) & ~63, np.uint16 if bd > 8 else np.uint8
        bs = 2 if bd > 8 else 1
        st = svtgpu.TfState(ctx, w, h)
        refs = [[np.pad(r.integers(0, 1 << bd, (h >> (p > 0), w >> (p > 0))).astype(dt), PAD >> (p > 0), mode="edge")
                 for p in range(3)] for _ in range(N_REFS)]
        motion = [m for _ in range(N_REFS) for m in ic.random_motion(r, st.nblk, w)]
        ma = (svtgpu.TfMotion * len(motion))(*[svtgpu.TfMotion.make(m["use64"], m["mv64"], m["split32"], m["split16"], m["mv32"],
                                                                    m["mv16"], m["mv8"]) for m in motion])
        dr = [[dev(a) for a in ref] for ref in refs]
        dp = [[dev(np.zeros((ah >> (p > 0), aw >> (p > 0)), dt)) for p in range(3)] for _ in range(N_REFS)]
        pr = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make(
            [t[p].data_ptr() + (PAD >> (p > 0)) * (a[p].shape[1] + 1) * bs for p in range(3)], [a[p].shape[1] for p in range(3)])
            for t, a in zip(dr, refs)])
        pp = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make([t.data_ptr() for t in d], [aw, aw >> 1, aw >> 1]) for d in dp])
        L = svtgpu.lib()
        run = lambda: svtgpu.check(L.svtgpu_tf_predict_frame(st.h, pr, N_REFS, PAD, PAD, ma, bd, 1, pp, None))
        for _ in range(args.warmup):
            run()
        ctx.synchronize()
        ms = [timed(stream, args.reps, run) for _ in range(3)]
        nbytes = N_REFS * ((w * h * 3 // 2) + (aw * ah * 3 // 2)) * bs + ctypes.sizeof(ma)
        got = [t.cpu().numpy().view(dt) for t in dp[0]]
        print(json.dumps({
            "metric": "tf_predict_hbm_fraction", "workload": "%dx%d %d-bit 4:2:0, %d references" % (w, h, bd, N_REFS),
            "reps": args.reps, "predict_ms": [round(v, 4) for v in ms], "bytes": nbytes,
            "gb_s": round(nbytes / (min(ms) * 1e-3) / 1e9, 1), "hbm_fraction": round(nbytes / (min(ms) * 1e-3) / HBM_PEAK, 4),
            "blocks_64_32_16_8": [sum(len([b for b in ic.blocks_of(m) if b[2] == s]) for m in motion) for s in (64, 32, 16, 8)],
            "sample_sum": int(sum(int(a.reshape(-1)[::97].sum()) for a in got)), "data": "synthetic"}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
