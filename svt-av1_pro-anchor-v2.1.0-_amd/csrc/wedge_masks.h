// wedge_masks.h — the 6-bit blending masks of AV1's wedge compound (COMPOUND_WEDGE): what svt_av1_init_wedge_masks
// (EbInterPrediction.c:1445-2132) builds and svt_aom_get_contiguous_soft_mask returns, as a function of the sample:
// value(w_log2, h_log2, index, sign, row, col).  Held to all 288 masks of the reference (nine sizes, sixteen indices, two
// signs) by tests/test_masked_compound.py, through the library and through a stand-alone host program.  Plain C++: no HIP
// in it, a host compiler can include it (as csrc/compound_weights.h); under hipcc the functions are also device functions.
// Everything is arithmetic on constants that fit registers: no table in memory, so the device needs no upload and no
// indexed constant read.
//
//   primary rows   the reference's three 64-entry rows are 0 up to entry 27, 64 from entry 36, and differ in the eight
//                  entries between: those eight bytes are one 64-bit constant per row.
//   primaries      OBLIQUE63 row i is the even (i even) or odd row shifted right by 16 - ((i + 1) >> 1) with its ends
//                  repeated; VERTICAL row i is the vertical row; OBLIQUE27 and HORIZONTAL are their transposes; OBLIQUE117
//                  is 64 - OBLIQUE63 mirrored left to right, OBLIQUE153 its transpose (init_wedge_primary_masks).
//   a block's mask the 64x64 primary of the codebook entry's direction read from (32 - y_offset * h / 8, 32 - x_offset * w / 8)
//                  (get_wedge_mask_inplace), complemented when sign != the entry's precomputed sign flip.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WEDGE_MASKS_FN __host__ __device__ inline
#else
#define WEDGE_MASKS_FN inline
#endif

namespace wedge_masks {

constexpr int kIndices   = 16; // 1 << wedge_params_lookup[bsize].bits
constexpr int kMaxAlpha  = 64; // 1 << WEDGE_WEIGHT_BITS = AOM_BLEND_A64_MAX_ALPHA
constexpr int kTotalBytes = 2 * kIndices * (64 + 2 * 128 + 2 * 256 + 256 + 2 * 512 + 1024); // all nine sizes: 100352

enum Direction { kHorizontal = 0, kVertical = 1, kOblique27 = 2, kOblique63 = 3, kOblique117 = 4, kOblique153 = 5 };

// entries 28 .. 35 of wedge_primary_oblique_even, _odd and wedge_primary_vertical, entry 28 in the low byte
constexpr uint64_t kRowEven = 0x3F3E3A2E1B0B0401ull; // 1 4 11 27 46 58 62 63
constexpr uint64_t kRowOdd  = 0x3F3C352512060201ull; // 1 2 6 18 37 53 60 63
constexpr uint64_t kRowVert = 0x403E392B15070200ull; // 0 2 7 21 43 57 62 64

struct Code {
    int direction, x_offset, y_offset;
};
// the three codebooks differ in entries 4 .. 7 only
#define WEDGE_MASKS_HEAD {kOblique27, 4, 4}, {kOblique63, 4, 4}, {kOblique117, 4, 4}, {kOblique153, 4, 4}
#define WEDGE_MASKS_TAIL                                                                                              \
    {kOblique27, 4, 2}, {kOblique27, 4, 6}, {kOblique153, 4, 2}, {kOblique153, 4, 6}, {kOblique63, 2, 4}, {kOblique63, 6, 4}, \
        {kOblique117, 2, 4}, {kOblique117, 6, 4}
constexpr Code kCodebookHgtW[kIndices] = { // wedge_codebook_16_hgtw: taller than wide
    WEDGE_MASKS_HEAD, {kHorizontal, 4, 2}, {kHorizontal, 4, 4}, {kHorizontal, 4, 6}, {kVertical, 4, 4}, WEDGE_MASKS_TAIL};
constexpr Code kCodebookHltW[kIndices] = { // wedge_codebook_16_hltw: wider than tall
    WEDGE_MASKS_HEAD, {kVertical, 2, 4}, {kVertical, 4, 4}, {kVertical, 6, 4}, {kHorizontal, 4, 4}, WEDGE_MASKS_TAIL};
constexpr Code kCodebookHeqW[kIndices] = { // wedge_codebook_16_heqw: square
    WEDGE_MASKS_HEAD, {kHorizontal, 4, 2}, {kHorizontal, 4, 6}, {kVertical, 2, 4}, {kVertical, 6, 4}, WEDGE_MASKS_TAIL};
#undef WEDGE_MASKS_HEAD
#undef WEDGE_MASKS_TAIL

// a codebook as one constant: entry i in bits 4 i .. 4 i + 3 of each of the three words
struct Packed {
    uint64_t direction, x_offset, y_offset;
};
constexpr Packed pack(const Code (&c)[kIndices]) {
    Packed p = {0, 0, 0};
    for (int i = 0; i < kIndices; i++) {
        p.direction |= (uint64_t)c[i].direction << (4 * i);
        p.x_offset |= (uint64_t)c[i].x_offset << (4 * i);
        p.y_offset |= (uint64_t)c[i].y_offset << (4 * i);
    }
    return p;
}
constexpr Packed kPackedHgtW = pack(kCodebookHgtW), kPackedHltW = pack(kCodebookHltW), kPackedHeqW = pack(kCodebookHeqW);

// wedge_signflip_lookup, bit i for index i: square sizes, 2:1 sizes (both ways), 8x32, 32x8
constexpr uint32_t kFlipSquare = 0xBBFF, kFlipTwoToOne = 0xBBEF, kFlip8x32 = 0xBAEF, kFlip32x8 = 0xABEF;

// wedge_params_lookup[bsize].bits > 0: 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32, 8x32, 32x8
WEDGE_MASKS_FN bool bits(int w_log2, int h_log2) { return w_log2 >= 3 && w_log2 <= 5 && h_log2 >= 3 && h_log2 <= 5; }

// entry t of a primary row (any integer: 0 before the row, 64 behind it, as the reference's shift_copy repeats the ends)
WEDGE_MASKS_FN int row_entry(uint64_t row, int t) {
    if (t < 28) return 0;
    if (t > 35) return kMaxAlpha;
    return (int)((row >> (8 * (t - 28))) & 0xFF);
}
// What a block's mask is made of.  Every primary is one row walked along a line: with (i, j) = (r, c), or (c, r) for the
// transposed directions, and j mirrored (63 - j) for the two whose primary is the complement of a mirrored OBLIQUE63, the
// value is entry j of the vertical row, or entry j - 16 + ((i + 1) >> 1) of the even / odd row by i's parity.  So a plan is
// four flags and the block's origin in the 64x64 primary, and a value is selects and shifts without a branch.
struct Plan {
    int transposed, mirrored, oblique, complement, r0, c0;
};
WEDGE_MASKS_FN Plan plan(int w_log2, int h_log2, int index, int sign) {
    const Packed   p = h_log2 > w_log2 ? kPackedHgtW : h_log2 < w_log2 ? kPackedHltW : kPackedHeqW;
    const uint32_t flips = h_log2 == w_log2 ? kFlipSquare
        : (w_log2 == 3 && h_log2 == 5)     ? kFlip8x32
        : (w_log2 == 5 && h_log2 == 3)     ? kFlip32x8
                                           : kFlipTwoToOne;
    const int sh = 4 * index, d = (int)((p.direction >> sh) & 15);
    const int woff = ((int)((p.x_offset >> sh) & 15) << w_log2) >> 3, hoff = ((int)((p.y_offset >> sh) & 15) << h_log2) >> 3;
    const int mirrored = d == kOblique117 || d == kOblique153;
    return Plan{d == kHorizontal || d == kOblique27 || d == kOblique153, mirrored, d >= kOblique27,
                (int)((sign ^ (flips >> index) ^ mirrored) & 1), 32 - hoff, 32 - woff};
}
WEDGE_MASKS_FN int plan_value(const Plan &p, int row, int col) {
    const int r = p.r0 + row, c = p.c0 + col, i = p.transposed ? c : r, j0 = p.transposed ? r : c, j = p.mirrored ? 63 - j0 : j0;
    const int v = row_entry(p.oblique ? ((i & 1) ? kRowOdd : kRowEven) : kRowVert, p.oblique ? j - 16 + ((i + 1) >> 1) : j);
    return p.complement ? kMaxAlpha - v : v;
}

// The mask value at (row, col) of a 2^w_log2 x 2^h_log2 block for wedge `index` (0 .. 15) and `sign` (0 / 1); the size has
// wedges (bits()).
WEDGE_MASKS_FN int value(int w_log2, int h_log2, int index, int sign, int row, int col) {
    return plan_value(plan(w_log2, h_log2, index, sign), row, col);
}

// the whole mask, w * h bytes with stride w
WEDGE_MASKS_FN void fill(int w_log2, int h_log2, int index, int sign, uint8_t *mask) {
    const Plan p = plan(w_log2, h_log2, index, sign);
    for (int y = 0; y < (1 << h_log2); y++)
        for (int x = 0; x < (1 << w_log2); x++) mask[(y << w_log2) + x] = (uint8_t)plan_value(p, y, x);
}

} // namespace wedge_masks
