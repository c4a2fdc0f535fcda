"""The temporal filter's filter half (svtgpu_tf_filter_frame, svtgpu_tf_estimate_noise_async) on the MI355X, timed with HIP
events after warm-up.

Workloads (synthetic, stated): a 1920x1080 8-bit and a 3840x2160 10-bit 4:2:0 picture with 6 predictor pictures (the
centre plus small noise), random split flags, motion vectors and block errors.  Reported as fractions of the HBM bandwidth
from the algorithmic bytes: the centre read once, every predictor picture read once, the output written once (the
64-aligned area, as the kernel filters whole blocks); the metadata upload (256 bytes per reference and block) is part of
the timed call.  The noise estimate reads the luma plane once.
tests/golden/gen_golden_tf.c --time runs the same workloads through the reference's C (and AVX2) on one host core.

    python3 scripts/tf_perf.py [--reps 100] [--warmup 10]
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
import tf_cases as tc  # noqa: E402

SHAPES = [(8, 1920, 1080), (10, 3840, 2160)]
N_REFS = 6
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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime takes the device before libsvtgpu's
    ctx = svtgpu.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    for bd, w, h in SHAPES:
        r = np.random.default_rng(0x5446 + bd)
        aw, ah, dt = (w + 63) & ~63, (h + 63) & ~63, tc.dtype_of(bd)
        centre = [r.integers(0, 1 << bd, (ah >> (p > 0), aw >> (p > 0))).astype(dt) for p in range(3)]
        refs = [[np.clip(c.astype(np.int32) + r.integers(-(k + 1) * 3, (k + 1) * 3 + 1, c.shape), 0, (1 << bd) - 1).astype(dt)
                 for c in centre] for k in range(N_REFS)]
        st = svtgpu.TfState(ctx, w, h)
        metas = tc.random_metas(r, N_REFS, st.nblk, bd)
        blocks = [svtgpu.TfBlock.make(m["split"], m["mv32"], m["mv16"], m["err32"], m["err16"]) for row in metas for m in row]
        dc, dr = [dev(a) for a in centre], [[dev(a) for a in ref] for ref in refs]
        do = [dev(np.zeros_like(a)) for a in centre]
        planes = lambda ts: svtgpu.TfPlanes.make([t.data_ptr() for t in ts], [a.shape[1] for a in centre])
        pc, po, pr = planes(dc), planes(do), (svtgpu.TfPlanes * N_REFS)(*[planes(t) for t in dr])
        ba = (svtgpu.TfBlock * len(blocks))(*blocks)
        prm = svtgpu.TfParams.make([6000000, 9000000, 12000000], 1080, 1, bd)
        L = svtgpu.lib()
        filt = lambda: svtgpu.check(L.svtgpu_tf_filter_frame(st.h, pc, pr, N_REFS, ba, prm, po, None))
        noise = lambda: st.estimate_noise_async(dc[0].data_ptr(), bd, aw, w, h)
        for _ in range(args.warmup):
            filt()
            noise()
        ctx.synchronize()
        ms_f = [timed(stream, args.reps, filt) for _ in range(3)]
        ms_n = [timed(stream, args.reps, noise) for _ in range(3)]
        bs = 2 if bd > 8 else 1
        bytes_f = (N_REFS + 2) * (aw * ah * 3 // 2) * bs
        bytes_n = w * h * bs
        got = [t.cpu().numpy().view(dt) for t in do]
        print(json.dumps({
            "metric": "tf_hbm_fraction", "workload": "%dx%d %d-bit 4:2:0, %d references" % (w, h, bd, N_REFS),
            "reps": args.reps, "filter_ms": [round(v, 4) for v in ms_f], "noise_ms": [round(v, 4) for v in ms_n],
            "filter_bytes": bytes_f, "noise_bytes": bytes_n,
            "filter_tb_s": round(bytes_f / (min(ms_f) * 1e-3) / 1e12, 3),
            "filter_hbm_fraction": round(bytes_f / (min(ms_f) * 1e-3) / HBM_PEAK, 3),
            "noise_hbm_fraction": round(bytes_n / (min(ms_n) * 1e-3) / HBM_PEAK, 3),
            "noise_fp16": st.read_noise(), "sample_sum": int(sum(int(a.reshape(-1)[::97].sum()) for a in got)),
            "data": "synthetic"}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
