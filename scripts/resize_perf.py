"""The non-normative frame resizer (svtgpu_resize_frame) on the MI355X, timed with HIP events after warm-up, beside the
project's streaming yardstick svtgpu_frame_convert in the same run.

Workloads (synthetic, stated): a 3840x2160 10-bit 4:2:0 picture of random samples resized to 2880x1620 (code 17: one
interpolation per direction), to 1920x1080 (denominator 16: one halving per direction) and to 2560x2160 (width only),
three planes each; the yardstick converts the 3840x2160 10-bit picture to 8 bits.  All are reported as fractions of the
HBM bandwidth from their algorithmic bytes: the source read once, the intermediate plane [src_h][dst_w] written and read
(none when only one direction changes), the destination written once.
tests/golden/gen_golden_resize.c --time runs the same three resizes through the reference's C on one host core.

    python3 scripts/resize_perf.py [--reps 200] [--warmup 10]
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

W, H, BD = 3840, 2160, 10
SHAPES = [(2880, 1620), (1920, 1080), (2560, 2160)]
HBM_PEAK = 8.0e12      # bytes/s, the MI355X's specified HBM3E bandwidth
HBM_COPY = 6.29e12     # bytes/s, a measured float4 copy on the same part


def timed(stream, reps, fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(stream):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime takes the device before libsvtgpu's
    ctx = svtgpu.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    r = np.random.default_rng(0x5253)
    src = svtgpu.Frame(ctx, W, H, BD)
    src.upload([r.integers(0, 1 << BD, (H >> (p > 0), W >> (p > 0))).astype(np.uint16) for p in range(3)])
    out8 = svtgpu.Frame(ctx, W, H, 8)
    convert = lambda: svtgpu.check(svtgpu.lib().svtgpu_frame_convert(src.h, out8.h, None))
    samples = W * H * 3 // 2
    bytes_cv = 2 * samples + samples
    for dw, dh in SHAPES:
        dst = svtgpu.Frame(ctx, (dw + 7) & ~7, (dh + 7) & ~7, BD)
        resize = lambda: svtgpu.resize(src, dst, W, H, dw, dh)
        for _ in range(args.warmup):
            resize()
            convert()
        ctx.synchronize()
        ms_rs, ms_cv = [], []
        for _ in range(3):  # alternate the two so both see the same machine state
            ms_rs.append(timed(stream, args.reps, resize))
            ms_cv.append(timed(stream, args.reps, convert))
        mid = dw * H * 3 // 2 if (dw != W and dh != H) else 0
        bytes_rs = 2 * (samples + 2 * mid + dw * dh * 3 // 2)
        t_rs, t_cv = min(ms_rs) * 1e-3, min(ms_cv) * 1e-3
        got = dst.download()
        print(json.dumps({
            "metric": "resize_hbm_fraction",
            "workload": "%dx%d -> %dx%d %d-bit 4:2:0, three planes" % (W, H, dw, dh, BD), "reps": args.reps,
            "resize_ms": [round(v, 4) for v in ms_rs], "convert_ms": [round(v, 4) for v in ms_cv],
            "resize_bytes": bytes_rs, "convert_bytes": bytes_cv,
            "resize_tb_s": round(bytes_rs / t_rs / 1e12, 3), "convert_tb_s": round(bytes_cv / t_cv / 1e12, 3),
            "resize_hbm_fraction": round(bytes_rs / t_rs / HBM_PEAK, 3),
            "convert_hbm_fraction": round(bytes_cv / t_cv / HBM_PEAK, 3),
            "resize_fraction_of_measured_copy": round(bytes_rs / t_rs / HBM_COPY, 3),
            "convert_fraction_of_measured_copy": round(bytes_cv / t_cv / HBM_COPY, 3),
            "sample_sum": int(sum(int(a[:(dh + (p > 0)) >> (p > 0), :(dw + (p > 0)) >> (p > 0)].reshape(-1)[::97].sum())
                                  for p, a in enumerate(got))), "data": "synthetic"}), flush=True)
        dst.close()


if __name__ == "__main__":
    main()
