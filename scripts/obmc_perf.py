"""The batched OBMC full-pel search (svtgpu_obmc_search) on the MI355X, timed with HIP events after warm-up.

Workload (synthetic, stated): every 16x16 block of a 1920x1080 8-bit picture (120 x 67 = 8040 items, one reference),
search_range 16 with diagonals, cost mode 0, start and centre MV 0, limits +-64.  The picture is two triangle waves,
each block's wsrc its own mask (2048 + 64 * (px + py)) times the picture displaced by up to +-12 samples, so the walks
run for several steps.  tests/golden/gen_golden_obmc.c --time runs the same item list through the reference's C walk
on one host core and prints the same checksum (sum of variance + 3 * col + 7 * row over the items).

    python3 scripts/obmc_perf.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "svt-av1_pro-anchor-v2.1.0-_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svtgpu  # noqa: E402

W, H, BW, BH = 1920, 1080, 16, 16


def tri(v):
    return np.minimum(2 * np.abs((v & 255) - 128), 255)


def workload():
    yy, xx = np.mgrid[0:H, 0:W]
    pic = ((tri(3 * xx + yy) + tri(5 * yy - xx + 1000)) >> 1).astype(np.uint8)
    pad = 32
    padded = np.pad(pic, pad, mode="edge").astype(np.int32)
    py, px = np.mgrid[0:BH, 0:BW]
    mask = (2048 + 64 * (px + py)).astype(np.int32)
    nbx, nby, n = W // BW, H // BH, BW * BH
    items, pool = [], np.empty((nby * nbx, 2, n), np.int32)
    for by in range(nby):
        for bx in range(nbx):
            dx, dy = (bx * 7 + by * 3) % 25 - 12, (bx * 5 + by * 11) % 25 - 12
            y0, x0 = by * BH + dy + pad, bx * BW + dx + pad
            i = by * nbx + bx
            pool[i, 0] = (mask * padded[y0:y0 + BH, x0:x0 + BW]).reshape(-1)
            pool[i, 1] = mask.reshape(-1)
            items.append(dict(ref=0, x=bx * BW, y=by * BH, w=BW, h=BH, mvp_col=0, mvp_row=0, ref_mv_col=0, ref_mv_row=0,
                              col_min=-64, col_max=64, row_min=-64, row_max=64, sad_per_bit=60, search_range=16,
                              search_diag=1, cost_mode=0, wm_offset=2 * n * i, cost_offset=0))
    return pic, items, pool.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime takes the device before libsvtgpu's
    ctx = svtgpu.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    pic, items, pool = workload()
    ref = svtgpu.Frame(ctx, W, H, 8)
    ref.upload([pic, np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)])
    b = svtgpu.ObmcBatch(ctx, W, H, 1, len(items))
    b.set_items(items, pool)
    for _ in range(args.warmup):
        b.search([ref])
    ctx.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(stream):
        ev[0].record()
        for _ in range(args.reps):
            b.search([ref])
        ev[1].record()
    ev[1].synchronize()
    ms = ev[0].elapsed_time(ev[1]) / args.reps
    r = b.read()
    col, row = r["mv_col"].astype(np.int64), r["mv_row"].astype(np.int64)
    print(json.dumps({
        "metric": "obmc_search_items_per_s",
        "workload": "1920x1080 8-bit, every 16x16 block, range 16 with diagonals, cost mode 0",
        "items": len(items), "reps": args.reps, "ms": round(ms, 4), "items_per_s": round(len(items) / (ms * 1e-3)),
        "moves": int(r["steps"].sum()), "chebyshev_moves": int(np.maximum(np.abs(col), np.abs(row)).sum()),
        "checksum": int((r["variance"].astype(np.int64) + 3 * col + 7 * row).sum()),
        "data": "synthetic"}), flush=True)
    b.close()


if __name__ == "__main__":
    main()
