// warp_params.h — the host-side parameters of AV1 warped-motion (affine) prediction, HIP-free: the warped filter table
// (193 rows of 8 taps, 7 fractional bits; the AV1 specification's Warped_Filters, the reference's svt_aom_warped_filter,
// EbWarpedMotion.c:56), the divisor table behind resolve_divisor_32 (:298-350), and svt_get_shear_params (:1082-1105): the
// four shear parameters alpha, beta, gamma, delta of a model and whether the 8-tap warp filter may run on it.
// warp.hip's entry points and kernels use it; tests/warp_params_check.cpp compiles it alone with g++; both tables and the
// shear parameters are held to the values the reference compiled by tests/test_warp.py (tests/golden/warp.bin).
//
// Finding the model -- svt_find_projection's least squares over the neighbours' motion vectors, svt_aom_select_samples,
// the global motion search -- stays on the host and is not here: the entry points take the six wmmat values as
// svt_warp_plane passes them (for ROTZOOM the caller has set [5] = [2] and [4] = -[3]).
//
// Form.  Every tap lies in [-22, 127], so a row is eight signed bytes in one 64-bit word, tap k in byte k; expand() makes
// the int16 rows (16 bytes each: one 128-bit read per row) at compile time.  Row r is the filter of offset (r - 64) / 64
// sample: rows 0 .. 63 for [-1, 0), 64 .. 127 for [0, 1), 128 .. 192 for [1, 2].  The divisor table is computed:
// entry f is 2^22 / (256 + f) rounded to nearest, f = 0 .. 256.
#pragma once
#include <cstdint>

#ifndef SVTGPU_OK
#define SVTGPU_OK 0
#define SVTGPU_ERR_INVALID_ARG (-1)
#endif

namespace warp_params {

constexpr int kModelPrecBits  = 16; // WARPEDMODEL_PREC_BITS: the fixed point of wmmat[2 .. 5] and of the projection
constexpr int kReduceBits     = 6;  // WARP_PARAM_REDUCE_BITS: the shear parameters are multiples of 1 << 6
constexpr int kDiffPrecBits   = 10; // WARPEDDIFF_PREC_BITS: model precision minus the table's 6 fractional bits
constexpr int kPixelShifts    = 64; // WARPEDPIXEL_PREC_SHIFTS: table rows per sample
constexpr int kFilterRows     = 3 * kPixelShifts + 1;
constexpr int kDivLutBits     = 8, kDivLutPrecBits = 14, kDivLutNum = 1 << kDivLutBits;

constexpr uint64_t kPackedRows[kFilterRows] = {
    0x00000000017f0000ull, 0x00000000027fff00ull, 0x000000ff047ffd01ull, 0x000001fe067efc01ull,
    0x000001fd087efb01ull, 0x000001fc0b7dfa01ull, 0x000001fc0d7cf901ull, 0x000001fb0f7bf802ull,
    0x000001fa127af702ull, 0x000001fa1479f602ull, 0x000002f91678f502ull, 0x000002f81977f402ull,
    0x000002f81b75f303ull, 0x000002f71d74f303ull, 0x000003f62072f203ull, 0x000002f62371f103ull,
    0x000003f5256ff103ull, 0x000003f5286df003ull, 0x000003f42a6cf003ull, 0x000003f32d6aef04ull,
    0x000003f32f68ef04ull, 0x000003f23266ef04ull, 0x000003f23464ef04ull, 0x000004f13762ee04ull,
    0x000003f13a60ee04ull, 0x000004f03c5eee04ull, 0x000004f03f5bee04ull, 0x000004f04159ee04ull,
    0x000004ef4457ee04ull, 0x000004ef4655ee04ull, 0x000004ef4952ee04ull, 0x000004ef4b50ee04ull,
    0x000004ee4e4eee04ull, 0x000004ee504bef04ull, 0x000004ee5249ef04ull, 0x000004ee5546ef04ull,
    0x000004ee5744ef04ull, 0x000004ee5941f004ull, 0x000004ee5b3ff004ull, 0x000004ee5e3cf004ull,
    0x000004ee603af103ull, 0x000004ee6237f104ull, 0x000004ef6434f203ull, 0x000004ef6632f203ull,
    0x000004ef682ff303ull, 0x000004ef6a2df303ull, 0x000003f06c2af403ull, 0x000003f06d28f503ull,
    0x000003f16f25f503ull, 0x000003f17123f602ull, 0x000003f27220f603ull, 0x000003f3741df702ull,
    0x000003f3751bf802ull, 0x000002f47719f802ull, 0x000002f57816f902ull, 0x000002f67914fa01ull,
    0x000002f77a12fa01ull, 0x000002f87b0ffb01ull, 0x000001f97c0dfc01ull, 0x000001fa7d0bfc01ull,
    0x000001fb7e08fd01ull, 0x000001fc7e06fe01ull, 0x000001fd7f04ff00ull, 0x000000ff7f020000ull,
    0x000000017f000000ull, 0x000000027fff0000ull, 0x0001fe047ffd0100ull, 0x0001fe067ffb0100ull,
    0x0001fd087efa0200ull, 0xff02fc0b7ef902ffull, 0xff02fb0d7df803ffull, 0xff03fa107cf603ffull,
    0xff03f9127bf504ffull, 0xff03f9147af404ffull, 0xff03f81779f304ffull, 0xff04f71978f205feull,
    0xff04f61b77f105ffull, 0xff04f51e76f005ffull, 0xff05f42174ef06feull, 0xff05f42372ef06feull,
    0xff05f32671ee06feull, 0xfe06f2296fed07feull, 0xfe06f12b6eed07feull, 0xfe06f12e6cec07feull,
    0xfe06f0316aec07feull, 0xfe07f03368eb07feull, 0xfe07ef3666eb07feull, 0xfe07ee3864eb08feull,
    0xfe07ee3b62ea08feull, 0xfe07ed3e60ea08feull, 0xfe07ed405eea08feull, 0xfe08ec435bea08feull,
    0xfe08ec4559ea08feull, 0xfe08eb4857ea08feull, 0xfe08eb4a54eb08feull, 0xfe08eb4d52ea08feull,
    0xfe08eb4f4feb08feull, 0xfe08ea524deb08feull, 0xfe08eb544aeb08feull, 0xfe08ea5748eb08feull,
    0xfe08ea5945ec08feull, 0xfe08ea5b43ec08feull, 0xfe08ea5e40ed07feull, 0xfe08ea603eed07feull,
    0xfe08ea623bee07feull, 0xfe08eb6438ee07feull, 0xfe07eb6636ef07feull, 0xfe07eb6833f007feull,
    0xfe07ec6a31f006feull, 0xfe07ec6c2ef106feull, 0xfe07ed6e2bf106feull, 0xfe07ed6f29f206feull,
    0xfe06ee7126f305ffull, 0xfe06ef7223f405ffull, 0xfe06ef7421f405ffull, 0xff05f0761ef504ffull,
    0xff05f1771bf604ffull, 0xfe05f27819f704ffull, 0xff04f37917f803ffull, 0xff04f47a14f903ffull,
    0xff04f57b12f903ffull, 0xff03f67c10fa03ffull, 0xff03f87d0dfb02ffull, 0xff02f97e0bfc02ffull,
    0x0002fa7e08fd0100ull, 0x0001fb7f06fe0100ull, 0x0001fd7f04fe0100ull, 0x0000ff7f02000000ull,
    0x0000007f01000000ull, 0x0000027fff000000ull, 0x00ff047ffd010000ull, 0x01fe067efc010000ull,
    0x01fd087efb010000ull, 0x01fc0b7dfa010000ull, 0x01fc0d7cf9010000ull, 0x01fb0f7bf8020000ull,
    0x01fa127af7020000ull, 0x01fa1479f6020000ull, 0x02f91678f5020000ull, 0x02f81977f4020000ull,
    0x02f81b75f3030000ull, 0x02f71d74f3030000ull, 0x03f62072f2030000ull, 0x02f62371f1030000ull,
    0x03f5256ff1030000ull, 0x03f5286df0030000ull, 0x03f42a6cf0030000ull, 0x03f32d6aef040000ull,
    0x03f32f68ef040000ull, 0x03f23266ef040000ull, 0x03f23464ef040000ull, 0x04f13762ee040000ull,
    0x03f13a60ee040000ull, 0x04f03c5eee040000ull, 0x04f03f5bee040000ull, 0x04f04159ee040000ull,
    0x04ef4457ee040000ull, 0x04ef4655ee040000ull, 0x04ef4952ee040000ull, 0x04ef4b50ee040000ull,
    0x04ee4e4eee040000ull, 0x04ee504bef040000ull, 0x04ee5249ef040000ull, 0x04ee5546ef040000ull,
    0x04ee5744ef040000ull, 0x04ee5941f0040000ull, 0x04ee5b3ff0040000ull, 0x04ee5e3cf0040000ull,
    0x04ee603af1030000ull, 0x04ee6237f1040000ull, 0x04ef6434f2030000ull, 0x04ef6632f2030000ull,
    0x04ef682ff3030000ull, 0x04ef6a2df3030000ull, 0x03f06c2af4030000ull, 0x03f06d28f5030000ull,
    0x03f16f25f5030000ull, 0x03f17123f6020000ull, 0x03f27220f6030000ull, 0x03f3741df7020000ull,
    0x03f3751bf8020000ull, 0x02f47719f8020000ull, 0x02f57816f9020000ull, 0x02f67914fa010000ull,
    0x02f77a12fa010000ull, 0x02f87b0ffb010000ull, 0x01f97c0dfc010000ull, 0x01fa7d0bfc010000ull,
    0x01fb7e08fd010000ull, 0x01fc7e06fe010000ull, 0x01fd7f04ff000000ull, 0x00ff7f0200000000ull,
    0x00ff7f0200000000ull,
};

struct FilterTable {
    int16_t row[kFilterRows][8];
};
constexpr FilterTable expand() {
    FilterTable t{};
    for (int r = 0; r < kFilterRows; r++)
        for (int k = 0; k < 8; k++) t.row[r][k] = (int16_t)(int8_t)(uint8_t)(kPackedRows[r] >> (8 * k));
    return t;
}
static constexpr __attribute__((aligned(16))) FilterTable kFilter = expand();

// 2^22 / (256 + f), rounded: 1 / (1 + f / 256) at kDivLutPrecBits
constexpr int div_lut(int f) { return ((1 << (kDivLutPrecBits + kDivLutBits)) + ((kDivLutNum + f) >> 1)) / (kDivLutNum + f); }

// resolve_divisor_32: 1 / d = y / 2^shift with y at 14 bits; d > 0
inline int resolve_divisor(uint32_t d, int *shift) {
    int msb = 31;
    while (!(d >> msb)) msb--;
    const int32_t e = (int32_t)(d - ((uint32_t)1 << msb));
    const int32_t f = msb > kDivLutBits ? (e + ((1 << (msb - kDivLutBits)) >> 1)) >> (msb - kDivLutBits) : e << (kDivLutBits - msb);
    *shift = msb + kDivLutPrecBits;
    return div_lut(f);
}

inline int64_t round_signed_64(int64_t v, int n) { // ROUND_POWER_OF_TWO_SIGNED_64
    const int64_t half = ((int64_t)1 << n) >> 1;
    return v < 0 ? -((-v + half) >> n) : (v + half) >> n;
}
inline int clamp_i16(int64_t v) { return v < INT16_MIN ? INT16_MIN : v > INT16_MAX ? INT16_MAX : (int)v; }
// the reduction to a multiple of 1 << kReduceBits, stored back into an int16_t as the reference does (32767 rounds to
// 32768 and wraps to -32768 there too)
inline int16_t reduce(int v) {
    const int half = (1 << kReduceBits) >> 1;
    const int r    = v < 0 ? -((-v + half) >> kReduceBits) : (v + half) >> kReduceBits;
    return (int16_t)(r * (1 << kReduceBits));
}
inline bool shear_allowed(int a, int b, int c, int d) { // is_affine_shear_allowed
    auto mag = [](int v) { return v < 0 ? -v : v; };
    return 4 * mag(a) + 7 * mag(b) < (1 << kModelPrecBits) && 4 * mag(c) + 4 * mag(d) < (1 << kModelPrecBits);
}

// svt_get_shear_params: 1 and abgd = {alpha, beta, gamma, delta} when the model is valid (mat[2] > 0) and its shears fit the
// 8-tap filter, else 0 (abgd then holds what the reference leaves in the model: untouched for mat[2] <= 0, the rejected
// parameters otherwise)
inline int shear_params(const int32_t mat[6], int16_t abgd[4]) {
    if (mat[2] <= 0) return 0; // is_affine_valid
    int           shift;
    const int64_t y = resolve_divisor((uint32_t)mat[2], &shift);
    const int     alpha = clamp_i16((int64_t)mat[2] - (1 << kModelPrecBits)), beta = clamp_i16(mat[3]);
    const int     gamma = clamp_i16((int)round_signed_64((int64_t)mat[4] * (1 << kModelPrecBits) * y, shift)); // the (int) is the reference's
    const int     delta = clamp_i16((int64_t)mat[5] - (int)round_signed_64((int64_t)mat[3] * mat[4] * y, shift) - (1 << kModelPrecBits));
    abgd[0] = reduce(alpha), abgd[1] = reduce(beta), abgd[2] = reduce(gamma), abgd[3] = reduce(delta);
    return shear_allowed(abgd[0], abgd[1], abgd[2], abgd[3]) ? 1 : 0;
}

} // namespace warp_params

// The two exports of include/svtgpu.h that need nothing but this header (defined in warp.hip).
extern "C" int svtgpu_warp_shear_params(const int32_t wmmat[6], int16_t abgd[4]);
extern "C" int svtgpu_warp_filter_table(const int16_t **table, int32_t *rows);
