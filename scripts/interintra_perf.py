"""The batched inter-intra predictor (svtgpu_interintra_predict_batch) and its four-mode distortion
(svtgpu_interintra_mode_sse_batch) on the MI355X, timed with HIP events after warm-up as scripts/obmc_pred_perf.py times the
OBMC predictor, beside the same list through svtgpu_obmc_predict_batch with empty neighbour lists: the plain
single-reference predictor, the yardstick.

Workloads (synthetic, stated): a 1920x1080 8-bit and a 3840x2160 10-bit 4:2:0 picture, 3 reference pictures, the inter-intra
fixture's tiling (all seven sizes, 18 blocks per 96 x 64) over the largest multiple of 96 x 64 inside the picture, MVs within
+-8 samples, drawn modes, every second block wedge, full neighbour counts except in row 0 / column 0:
  interintra  svtgpu_interintra_predict_batch, luma and chroma;
  plain       the same blocks through svtgpu_obmc_predict_batch with n_above = n_left = 0;
  mode_sse    svtgpu_interintra_mode_sse_batch on the same blocks (luma, four modes).
The metadata upload (for inter-intra with the edge pool) is part of every timed call.  Median of 3 x `reps` calls.

    python3 scripts/interintra_perf.py [--reps 30] [--warmup 5]
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

import svtgpu  # noqa: E402
from tf_predict_perf import dev, timed  # noqa: E402

SHAPES = [(8, 1920, 1080), (10, 3840, 2160)]
N_REFS = 3
PAD = 160
TILING = [(0, 0, 32, 32), (32, 0, 32, 16), (32, 16, 16, 16), (48, 16, 16, 8), (48, 24, 8, 8), (56, 24, 8, 8), (64, 0, 16, 32),
          (80, 0, 8, 16), (88, 0, 8, 16), (80, 16, 16, 16), (0, 32, 16, 32), (16, 32, 32, 32), (48, 32, 32, 16), (48, 48, 16, 16),
          (64, 48, 16, 8), (64, 56, 8, 8), (72, 56, 8, 8), (80, 32, 16, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime takes the device before libsvtgpu's
    ctx = svtgpu.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    L = svtgpu.lib()
    for bd, w, h in SHAPES:
        r = np.random.default_rng(0x1149 + bd)
        dt, bs = (np.uint16, 2) if bd > 8 else (np.uint8, 1)
        st = svtgpu.TfState(ctx, w, h)
        refs = [[np.pad(r.integers(0, 1 << bd, (h >> (p > 0), w >> (p > 0))).astype(dt), PAD >> (p > 0), mode="edge")
                 for p in range(3)] for _ in range(N_REFS)]
        ii, plain, n_edges = [], [], 0
        for ty in range(h // 64):
            for tx in range(w // 96):
                for k, (bx, by, bw, bh) in enumerate(TILING):
                    x, y, mv, ref = bx + 96 * tx, by + 64 * ty, r.integers(-64, 65, 2), int(r.integers(0, N_REFS))
                    fx, fy = int(r.integers(0, 4)), int(r.integers(0, 4))
                    nt, nl = (bw if y else 0), (bh if x else 0)
                    ii.append(svtgpu.InterIntraBlock.make(x, y, bw, bh, ref, mv, fx, fy, int(r.integers(0, 4)), k & 1, int(r.integers(0, 16)),
                                                          (nt, nt // 2), (nl, nl // 2), n_edges))
                    plain.append(svtgpu.ObmcBlock.make(x, y, bw, bh, ref, mv, fx, fy))
                    n_edges += 2 * (bw + bh)
        edges = r.integers(0, 1 << bd, n_edges).astype(dt)
        dr = [[dev(a) for a in ref] for ref in refs]
        dp = [dev(np.zeros((h >> (p > 0), w >> (p > 0)), dt)) for p in range(3)]
        src = dev(refs[0][0][PAD:PAD + h, PAD:PAD + w].copy())
        sse = torch.zeros((len(ii), 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        pr = (svtgpu.TfPlanes * N_REFS)(*[svtgpu.TfPlanes.make(
            [t[p].data_ptr() + (PAD >> (p > 0)) * (a[p].shape[1] + 1) * bs for p in range(3)], [a[p].shape[1] for p in range(3)])
            for t, a in zip(dr, refs)])
        pp = svtgpu.TfPlanes.make([t.data_ptr() for t in dp], [w, w >> 1, w >> 1])
        what = "%dx%d %d-bit 4:2:0, %d blocks over %dx%d, %d references, half wedge" % (w, h, bd, len(ii), w // 96 * 96, h // 64 * 64, N_REFS)
        ia, oa = (svtgpu.InterIntraBlock * len(ii))(*ii), (svtgpu.ObmcBlock * len(plain))(*plain)
        runs = {
            "plain": lambda: svtgpu.check(L.svtgpu_obmc_predict_batch(st.h, pr, N_REFS, PAD, PAD, oa, len(plain), bd, 1, ctypes.byref(pp), None)),
            "interintra": lambda: svtgpu.check(L.svtgpu_interintra_predict_batch(st.h, pr, N_REFS, PAD, PAD, ia, len(ii), edges.ctypes.data,
                                                                                 n_edges, bd, 1, ctypes.byref(pp), None)),
            "mode_sse": lambda: svtgpu.check(L.svtgpu_interintra_mode_sse_batch(st.h, pr, N_REFS, PAD, PAD, ia, len(ii), edges.ctypes.data,
                                                                                n_edges, bd, src.data_ptr(), w, sse.data_ptr(), None)),
        }
        med = {}
        for name in ("plain", "interintra", "mode_sse"):
            run = runs[name]
            for _ in range(args.warmup):
                run()
            ctx.synchronize()
            ms = [timed(stream, args.reps, run) for _ in range(3)]
            med[name] = statistics.median(ms)
            print(json.dumps({"metric": "interintra_ms", "variant": name, "workload": what, "reps": args.reps,
                              "ms": [round(v, 4) for v in ms], "median_ms": round(med[name], 4), "edge_pool_bytes": n_edges * bs,
                              "data": "synthetic"}), flush=True)
        print(json.dumps({"metric": "interintra_over_plain", "workload": what, "ratio": round(med["interintra"] / med["plain"], 3)}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
