"""The batched masked compound predictor (svtgpu_masked_compound_predict_batch) on the MI355X, timed with HIP events after
warm-up, beside svtgpu_compound_predict_batch on the same geometry.

Workloads (synthetic, stated): scripts/compound_perf.py's -- a 1920x1080 8-bit and a 3840x2160 10-bit 4:2:0 picture, 3 padded
reference pictures (border 160), the compound fixture's tiling (all 17 sizes, 23 blocks per 256 x 192) over the largest
multiple of 256 x 192 inside the picture, filters mixed, MVs within +-64 samples -- run three ways in one process:
  wedge     every block COMPOUND_WEDGE, indices and signs in turn; a block larger than 32 in a direction is cut into pieces of
            at most 32 there (wedges exist up to 32x32), so the list has more blocks and the same samples;
  diffwtd   every block COMPOUND_DIFFWTD, mask types in turn, the tiling as it is;
  average   svtgpu_compound_predict_batch as COMPOUND_AVERAGE on the tiling as it is: the yardstick.
The metadata upload (blocks and the host-built item lists) is part of the timed call.  Median and best of 3 x `reps` calls.
tests/golden/gen_golden_masked_compound.c --time runs the wedge and DIFFWTD lists through the reference's C on one host core.

    python3 scripts/masked_compound_perf.py [--reps 50] [--warmup 10]
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
        r = np.random.default_rng(0x4D43 + bd)
        dt, bs = (np.uint16, 2) if bd > 8 else (np.uint8, 1)
        st = svtgpu.TfState(ctx, w, h)
        refs = [[np.pad(r.integers(0, 1 << bd, (h >> (p > 0), w >> (p > 0))).astype(dt), PAD >> (p > 0), mode="edge")
                 for p in range(3)] for _ in range(N_REFS)]
        lists = {"wedge": [], "diffwtd": [], "average": []}
        for ty in range(h // 192):
            for tx in range(w // 256):
                for b in tiling:
                    mv, r0, r1 = r.integers(-512, 513, 4), int(r.integers(0, 3)), int(r.integers(0, 3))
                    x, y = b["x"] + 256 * tx, b["y"] + 192 * ty
                    lists["average"].append(svtgpu.CompoundBlock.make(x, y, b["w"], b["h"], r0, r1, mv[:2], mv[2:], b["fx"], b["fy"]))
                    n = len(lists["diffwtd"])
                    lists["diffwtd"].append(svtgpu.MaskedCompoundBlock.make(x, y, b["w"], b["h"], r0, r1, mv[:2], mv[2:], b["fx"], b["fy"],
                                                                            1, mask_type=n & 1))
                    cw, ch = min(b["w"], 32), min(b["h"], 32)
                    for oy in range(0, b["h"], ch):
                        for ox in range(0, b["w"], cw):
                            n = len(lists["wedge"])
                            lists["wedge"].append(svtgpu.MaskedCompoundBlock.make(x + ox, y + oy, cw, ch, r0, r1, mv[:2], mv[2:], b["fx"],
                                                                                  b["fy"], 0, n & 15, (n >> 4) & 1))
        dr = [[dev(a) for a in ref] for ref in refs]
        dp = [dev(np.zeros((h >> (p > 0), w >> (p > 0)), dt)) for p in range(3)]
        pr = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make(
            [t[p].data_ptr() + (PAD >> (p > 0)) * (a[p].shape[1] + 1) * bs for p in range(3)], [a[p].shape[1] for p in range(3)])
            for t, a in zip(dr, refs)])
        pp = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], [w, w >> 1, w >> 1])
        for name in ("average", "wedge", "diffwtd"):
            blocks = lists[name]
            if name == "average":
                ba = (svtgpu.CompoundBlock * len(blocks))(*blocks)
                run = lambda: svtgpu.check(L.svtgpu_compound_predict_batch(st.h, pr, N_REFS, PAD, PAD, ba, len(blocks), bd, 1,
                                                                           ctypes.byref(pp), None))
            else:
                ba = (svtgpu.MaskedCompoundBlock * len(blocks))(*blocks)
                run = lambda: svtgpu.check(L.svtgpu_masked_compound_predict_batch(st.h, pr, N_REFS, PAD, PAD, ba, len(blocks), bd, 1,
                                                                                  ctypes.byref(pp), None))
            for _ in range(args.warmup):
                run()
            ctx.synchronize()
            ms = [timed(stream, args.reps, run) for _ in range(3)]
            outputs = sum((1 << b.w_log2) * (1 << b.h_log2) * 3 // 2 for b in blocks)
            got = [t.cpu().numpy().view(dt) for t in dp]
            print(json.dumps({
                "metric": "masked_compound_predict_ms", "variant": name, "workload": "%dx%d %d-bit 4:2:0, %d blocks over %dx%d, "
                "%d references" % (w, h, bd, len(blocks), w // 256 * 256, h // 192 * 192, N_REFS), "reps": args.reps,
                "predict_ms": [round(v, 4) for v in ms], "median_ms": round(statistics.median(ms), 4), "output_samples": outputs,
                "ps_per_filtered_sample": round(statistics.median(ms) * 1e9 / (2 * outputs), 2),
                "sample_sum": int(sum(int(a.reshape(-1)[::97].sum()) for a in got)), "data": "synthetic"}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
