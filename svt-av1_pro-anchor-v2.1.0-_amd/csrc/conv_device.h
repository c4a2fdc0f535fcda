// conv_device.h — the scalar device helpers the convolution kernels share: interp.hip, tf_search.hip, the compound
// family (compound_tile.h) and warp.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace conv_device {

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ int clip_bd(int v, int bd) {
    const int m = (1 << bd) - 1;
    return v < 0 ? 0 : v > m ? m : v;
}
__device__ __forceinline__ int round_shift(int v, int n) { return (v + ((1 << n) >> 1)) >> n; } // ROUND_POWER_OF_TWO
// the wave's LDS stores before its LDS loads: in order within a wave, the compiler must keep them so
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace conv_device
