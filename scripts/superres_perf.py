"""The super-resolution upscale (svtgpu_superres_upscale_frame) on the MI355X, timed with HIP events after warm-up,
beside the project's streaming yardstick svtgpu_frame_convert in the same run.

Workload (synthetic, stated): a 2560x2160 10-bit 4:2:0 picture of random samples upscaled to 3840x2160 (denominator 12),
three planes; the yardstick converts the 3840x2160 10-bit result to 8 bits.  Both are reported as fractions of the HBM
bandwidth from their algorithmic bytes (every source sample read once, every destination sample written once).
tests/golden/gen_golden_superres.c --time runs the same upscale through the reference's C on one host core.

    python3 scripts/superres_perf.py [--reps 200] [--warmup 10]
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

FW, UW, H, BD = 2560, 3840, 2160, 10
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
    r = np.random.default_rng(0x5352)
    src = svtgpu.Frame(ctx, FW, H, BD)
    src.upload([r.integers(0, 1 << BD, (H >> (p > 0), FW >> (p > 0))).astype(np.uint16) for p in range(3)])
    up, out8 = svtgpu.Frame(ctx, UW, H, BD), svtgpu.Frame(ctx, UW, H, 8)
    upscale = lambda: svtgpu.superres_upscale(src, up, FW, UW)
    convert = lambda: svtgpu.check(svtgpu.lib().svtgpu_frame_convert(up.h, out8.h, None))
    for _ in range(args.warmup):
        upscale()
        convert()
    ctx.synchronize()
    # alternate the two so both see the same machine state
    ms_up, ms_cv = [], []
    for _ in range(3):
        ms_up.append(timed(stream, args.reps, upscale))
        ms_cv.append(timed(stream, args.reps, convert))
    samples_in, samples_out = FW * H * 3 // 2, UW * H * 3 // 2
    bytes_up = 2 * samples_in + 2 * samples_out
    bytes_cv = 2 * samples_out + samples_out
    t_up, t_cv = min(ms_up) * 1e-3, min(ms_cv) * 1e-3
    got = up.download()
    print(json.dumps({
        "metric": "superres_upscale_hbm_fraction",
        "workload": "%dx%d -> %dx%d %d-bit 4:2:0, three planes" % (FW, H, UW, H, BD), "reps": args.reps,
        "upscale_ms": [round(v, 4) for v in ms_up], "convert_ms": [round(v, 4) for v in ms_cv],
        "upscale_bytes": bytes_up, "convert_bytes": bytes_cv,
        "upscale_tb_s": round(bytes_up / t_up / 1e12, 3), "convert_tb_s": round(bytes_cv / t_cv / 1e12, 3),
        "upscale_hbm_fraction": round(bytes_up / t_up / HBM_PEAK, 3),
        "convert_hbm_fraction": round(bytes_cv / t_cv / HBM_PEAK, 3),
        "upscale_fraction_of_measured_copy": round(bytes_up / t_up / HBM_COPY, 3),
        "convert_fraction_of_measured_copy": round(bytes_cv / t_cv / HBM_COPY, 3),
        "sample_sum": int(sum(int(a.reshape(-1)[::97].sum()) for a in got)), "data": "synthetic"}), flush=True)


if __name__ == "__main__":
    main()
