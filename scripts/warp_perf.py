"""The batched warped-motion predictor (svtgpu_warp_predict_batch) on the MI355X, timed with HIP events after warm-up, beside
svtgpu_compound_predict_batch on the same geometry.

Workloads (synthetic, stated): a 1920x1080 8-bit and a 3840x2160 10-bit 4:2:0 picture, 3 reference pictures, the compound
fixture's tiling (all 17 sizes, 23 blocks per 256 x 192) over the largest multiple of 256 x 192 inside the picture, run three
ways in one process:
  warp1     every block warped from one reference, small non-zero shears, translations within +-8 samples;
  warp2     every block warped from two references and averaged;
  average   svtgpu_compound_predict_batch as COMPOUND_AVERAGE on the same tiling (border 160): the yardstick.
Blocks of the tiling that are not at a multiple of 8 do not occur (it is built from sizes of 8 and up).  The metadata upload
(blocks and the host-built item lists) is part of the timed call.  Median and best of 3 x `reps` calls.

    python3 scripts/warp_perf.py [--reps 50] [--warmup 10]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "svt-av1_pro-anchor-v2.1.0-_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import compound_cases as cc  # noqa: E402
import svtgpu  # noqa: E402
from tf_predict_perf import dev, timed  # noqa: E402

SHAPES = [(8, 1920, 1080), (10, 3840, 2160)]
N_REFS = 3
PAD = 160


def model(r):
    return [int(r.integers(-8 << 16, 8 << 16)), int(r.integers(-8 << 16, 8 << 16)), 65536 + int(r.integers(-2000, 2001)),
            int(r.integers(-1500, 1501)), int(r.integers(-1500, 1501)), 65536 + int(r.integers(-2000, 2001))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime takes the device before libsvtgpu's
    ctx = svtgpu.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    tiling = cc.batch_cases()[0]["blocks"]
    L = svtgpu.lib()
    for bd, w, h in SHAPES:
        r = np.random.default_rng(0x5750 + bd)
        dt, bs = (np.uint16, 2) if bd > 8 else (np.uint8, 1)
        st = svtgpu.TfState(ctx, w, h)
        refs = [[np.pad(r.integers(0, 1 << bd, (h >> (p > 0), w >> (p > 0))).astype(dt), PAD >> (p > 0), mode="edge")
                 for p in range(3)] for _ in range(N_REFS)]
        lists = {"warp1": [], "warp2": [], "average": []}
        for ty in range(h // 192):
            for tx in range(w // 256):
                for b in tiling:
                    mv, r0, r1 = r.integers(-64, 65, 4), int(r.integers(0, 3)), int(r.integers(0, 3))
                    x, y = b["x"] + 256 * tx, b["y"] + 192 * ty
                    m0, m1 = model(r), model(r)
                    lists["average"].append(svtgpu.CompoundBlock.make(x, y, b["w"], b["h"], r0, r1, mv[:2], mv[2:], b["fx"], b["fy"]))
                    lists["warp1"].append(svtgpu.WarpBlock.make(x, y, b["w"], b["h"], r0, m0))
                    lists["warp2"].append(svtgpu.WarpBlock.make(x, y, b["w"], b["h"], r0, m0, r1, m1))
        dr = [[dev(a) for a in ref] for ref in refs]
        dp = [dev(np.zeros((h >> (p > 0), w >> (p > 0)), dt)) for p in range(3)]
        pr = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make(
            [t[p].data_ptr() + (PAD >> (p > 0)) * (a[p].shape[1] + 1) * bs for p in range(3)], [a[p].shape[1] for p in range(3)])
            for t, a in zip(dr, refs)])
        pp = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], [w, w >> 1, w >> 1])
        for name in ("average", "warp1", "warp2"):
            blocks = lists[name]
            if name == "average":
                ba = (svtgpu.CompoundBlock * len(blocks))(*blocks)
                run = lambda: svtgpu.check(L.svtgpu_compound_predict_batch(st.h, pr, N_REFS, PAD, PAD, ba, len(blocks), bd, 1,
                                                                           ctypes.byref(pp), None))
            else:
                ba = (svtgpu.WarpBlock * len(blocks))(*blocks)
                run = lambda: svtgpu.check(L.svtgpu_warp_predict_batch(st.h, pr, N_REFS, ba, len(blocks), bd, 1, ctypes.byref(pp), None))
            for _ in range(args.warmup):
                run()
            ctx.synchronize()
            ms = [timed(stream, args.reps, run) for _ in range(3)]
            # the warp writes no chroma for blocks below 16 in a dimension
            outputs = sum((1 << b.w_log2) * (1 << b.h_log2) * (3 if name == "average" or min(b.w_log2, b.h_log2) >= 4 else 2) // 2
                          for b in blocks)
            passes = 1 if name == "warp1" else 2
            got = [t.cpu().numpy().view(dt) for t in dp]
            print(json.dumps({
                "metric": "warp_predict_ms", "variant": name, "workload": "%dx%d %d-bit 4:2:0, %d blocks over %dx%d, "
                "%d references" % (w, h, bd, len(blocks), w // 256 * 256, h // 192 * 192, N_REFS), "reps": args.reps,
                "predict_ms": [round(v, 4) for v in ms], "median_ms": round(statistics.median(ms), 4), "output_samples": outputs,
                "ps_per_filtered_sample": round(statistics.median(ms) * 1e9 / (passes * outputs), 2),
                "sample_sum": int(sum(int(a.reshape(-1)[::97].sum()) for a in got)), "data": "synthetic"}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
