// conv_device.h — the scalar device helpers the prediction kernels share: interp.hip, tf_search.hip, the tile kernels
// (compound_tile.h) and warp.hip.  The MV clamp is pred_plan.h's, which the host tests too.
#pragma once
#include <hip/hip_runtime.h>

#include "pred_plan.h"

namespace conv_device {

using pred_plan::clamped_mv;

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ int clip_bd(int v, int bd) {
    const int m = (1 << bd) - 1;
    return v < 0 ? 0 : v > m ? m : v;
}
__device__ __forceinline__ int round_shift(int v, int n) { return (v + ((1 << n) >> 1)) >> n; } // ROUND_POWER_OF_TWO
// The tail of every compound: `value` the average, distance-weighted sum or blend of two CONV_BUF_TYPE values; removes
// the two-term offset, rounds by 14 - round_0 - round_1 and clips to the bit depth.
__device__ __forceinline__ int compound_finish(int value, int r0, int r1, int bd) {
    const int offset_bits = bd + 14 - r0;
    value -= (1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1));
    return clip_bd(round_shift(value, 14 - r0 - r1), bd);
}
// jnt_convolve's second pass and warp_affine's compound branch: the average or the distance-weighted sum, finished
__device__ __forceinline__ int compound_average(int first, int second, int dist_wtd, int fwd, int bck, int r0, int r1, int bd) {
    const int sum = dist_wtd ? (first * fwd + second * bck) >> pred_plan::kDistPrecisionBits : (first + second) >> 1;
    return compound_finish(sum, r0, r1, bd);
}
// the wave's LDS stores before its LDS loads: in order within a wave, the compiler must keep them so
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace conv_device
