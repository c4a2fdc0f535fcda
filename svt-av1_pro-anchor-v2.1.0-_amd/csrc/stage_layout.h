// stage_layout.h — the arithmetic of a staging buffer: how far a grow-only buffer grows, and where the regions of one
// reservation lie.  The per-thread stage of the RTCD shims (svtgpu_stage_reserve, runtime.hip) and the frame paths'
// layouts (lr_plan.h) both carve with it.  Integer arithmetic only: no HIP runtime, so a plain C++17 compiler builds it
// too (tests/stage_layout_check.cpp).
#pragma once
#include <cstddef>

// every carved region starts on a multiple of this (the strictest any user needs: the frame paths' 256-byte rows)
constexpr size_t kStageAlign = 256;

// The capacity a grow-only buffer takes when `need` bytes no longer fit: half as much again, in whole 4 KiB pages, so a
// run of slightly larger blocks reallocates once.
inline size_t stage_grown_capacity(size_t need) { return (need + (need >> 1) + 0xfff) & ~(size_t)0xfff; }
// the capacity after a reservation of `need` bytes from a buffer of `cap`: unchanged while the need fits
inline size_t stage_capacity_for(size_t cap, size_t need) { return need > cap ? stage_grown_capacity(need) : cap; }

// Adds up the regions of one buffer: c(bytes) is the offset of the next region, c.off the bytes carved so far.
struct Carver {
    size_t off = 0;
    size_t operator()(size_t bytes) {
        const size_t o = off;
        off += (bytes + kStageAlign - 1) & ~(kStageAlign - 1);
        return o;
    }
};
