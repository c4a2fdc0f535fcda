// interintra_plan_check.cpp — csrc/interintra_plan.h without HIP: every validation boundary (one case just inside, one just
// outside), the DC division against plain "/", the edge preparation's corner cases, every plane tile's edges inside its LDS
// slice, and the mask tables -- smooth masks of all 10 plane sizes x 4 modes, wedge masks of a plane for the seven sizes --
// printed for tests/test_interintra_plan_header.py, which holds them to tests/interintra_cases.py.  Built with plain g++.
#include <cstdio>
#include <cstdlib>

#include "../svt-av1_pro-anchor-v2.1.0-_amd/csrc/interintra_plan.h"

using namespace interintra_plan;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static const int kPlaneSizes[10][2] = {{4, 4}, {4, 8}, {8, 4}, {8, 8}, {8, 16}, {16, 8}, {16, 16}, {16, 32}, {32, 16}, {32, 32}};

static SvtGpuInterIntraBlock block(int w, int h) {
    SvtGpuInterIntraBlock b;
    memset(&b, 0, sizeof b);
    b.w_log2 = (uint8_t)log2_of(w), b.h_log2 = (uint8_t)log2_of(h);
    return b;
}

int main() {
    static_assert(sizeof(SvtGpuInterIntraBlock) == 32, "SvtGpuInterIntraBlock is 32 bytes");
    // the seven sizes, and nothing else of 4 .. 128
    int allowed = 0;
    for (int wl = 2; wl <= 7; wl++)
        for (int hl = 2; hl <= 7; hl++) {
            bool in = false;
            for (auto &s : kSizes) in |= s[0] == (1 << wl) && s[1] == (1 << hl);
            CHECK(size_allowed(wl, hl) == in);
            allowed += in;
        }
    CHECK(allowed == 7);
    for (auto &s : kPlaneSizes) CHECK(plane_size_ok(s[0], s[1]));
    CHECK(!plane_size_ok(4, 16) && !plane_size_ok(2, 4) && !plane_size_ok(64, 32) && !plane_size_ok(8, 12) && !plane_size_ok(0, 8));

    // validation boundaries: inside, then just outside
    {
        SvtGpuInterIntraBlock b = block(16, 32);
        const int             need = edge_samples(4, 5, 3);
        CHECK(need == 96 && edge_samples(4, 5, 1) == 48);
        CHECK(edge_plane_offset(4, 5, 0) == 0 && edge_plane_offset(4, 5, 1) == 48 && edge_plane_offset(4, 5, 2) == 72);
        b.mode = 3, b.use_wedge = 1, b.wedge_index = 15, b.filter_x = 3, b.filter_y = 3;
        b.n_top[0] = 16, b.n_top[1] = 8, b.n_left[0] = 32, b.n_left[1] = 16, b.edge_offset = 10;
        CHECK(block_ok(b, 3, 10 + need, true) && !block_ok(b, 3, 10 + need - 1, true));
        CHECK(block_ok(b, 1, 10 + 48, true) && !block_ok(b, 1, 10 + 47, true)); // luma only: the chroma parts need not exist
        SvtGpuInterIntraBlock c = b;
        c.edge_offset = 0;
        CHECK(block_ok(c, 3, need, true));
        c.edge_offset = -1;
        CHECK(!block_ok(c, 3, 1000, true));
        c = b, c.mode = 4;
        CHECK(!block_ok(c, 3, 1000, true) && block_ok(c, 3, 1000, false)); // the distortion entry does not look at the mode
        c = b, c.use_wedge = 2;
        CHECK(!block_ok(c, 3, 1000, true) && block_ok(c, 3, 1000, false));
        c = b, c.wedge_index = 16;
        CHECK(!block_ok(c, 3, 1000, true) && block_ok(c, 3, 1000, false));
        c = b, c.filter_x = 4;
        CHECK(!block_ok(c, 3, 1000, true));
        c = b, c.filter_y = 4;
        CHECK(!block_ok(c, 3, 1000, false));
        c = b, c.n_top[0] = 17;
        CHECK(!block_ok(c, 3, 1000, true));
        c = b, c.n_left[0] = 33;
        CHECK(!block_ok(c, 3, 1000, true));
        c = b, c.n_top[1] = 9;
        CHECK(!block_ok(c, 3, 1000, true) && block_ok(c, 1, 1000, true)); // a chroma count counts with chroma only
        c = b, c.n_left[1] = 17;
        CHECK(!block_ok(c, 3, 1000, true) && block_ok(c, 1, 1000, true));
        for (int k = 0; k < 8; k++) {
            c = b, c.reserved[k] = 1;
            CHECK(!block_ok(c, 3, 1000, true));
        }
        c = b, c.w_log2 = 3, c.h_log2 = 5; // 8x32: a wedge size, not an inter-intra size
        CHECK(!block_ok(c, 1, 1000, true));
        c = b, c.n_top[0] = 0, c.n_left[0] = 0, c.n_top[1] = 0, c.n_left[1] = 0;
        CHECK(block_ok(c, 3, 1000, true));
    }

    // the DC division: every reachable sum (12-bit samples, the shims' widest) of every plane size
    for (auto &s : kPlaneSizes) {
        const int wl = log2_of(s[0]), hl = log2_of(s[1]), n = s[0] + s[1];
        for (int sum = 0; sum <= n * 4095; sum++) CHECK(dc_divide(sum, wl, hl) == (sum + (n >> 1)) / n);
        CHECK(dc_value(kDcTop, 7 * s[0] + (s[0] >> 1), 99999, wl, hl, 8) == 8 && dc_value(kDcLeft, 99999, 7 * s[1] + (s[1] >> 1) - 1, wl, hl, 8) == 7);
        CHECK(dc_value(kDc128, 5, 5, wl, hl, 8) == 128 && dc_value(kDc128, 5, 5, wl, hl, 10) == 512);
    }
    CHECK(dc_variant(0, 0) == kDc128 && dc_variant(3, 0) == kDcTop && dc_variant(0, 1) == kDcLeft && dc_variant(8, 8) == kDcBoth);

    // the edge preparation
    {
        const uint16_t above[8] = {10, 11, 12, 13, 14, 15, 16, 17}, left[8] = {20, 21, 22, 23, 24, 25, 26, 27};
        CHECK(prepared_above(above, left, 8, 8, 10, 7) == 17 && prepared_above(above, left, 3, 8, 10, 2) == 12);
        CHECK(prepared_above(above, left, 3, 8, 10, 3) == 12 && prepared_above(above, left, 3, 8, 10, 7) == 12); // the last one repeated
        CHECK(prepared_above(above, left, 0, 5, 10, 4) == 20 && prepared_above(above, left, 0, 0, 10, 4) == 511 &&
              prepared_above(above, left, 0, 0, 8, 0) == 127);
        CHECK(prepared_left(above, left, 8, 8, 10, 7) == 27 && prepared_left(above, left, 8, 1, 10, 7) == 20);
        CHECK(prepared_left(above, left, 2, 0, 10, 6) == 10 && prepared_left(above, left, 0, 0, 10, 6) == 513 &&
              prepared_left(above, left, 0, 0, 8, 0) == 129);
        CHECK(constant_fill(kVPred, 0, 8) && !constant_fill(kVPred, 1, 0) && constant_fill(kHPred, 8, 0) && !constant_fill(kHPred, 0, 1));
        CHECK(!constant_fill(kDcPred, 0, 0) && !constant_fill(kSmoothPred, 0, 0));
    }
    // SMOOTH at the corners: weights 255 / 256 at (0, 0), the block's last weights at the far corner
    CHECK(smooth_value(100, 100, 100, 100, 8, 8, 3, 5) == 100);
    CHECK(smooth_value(1023, 0, 0, 0, 4, 4, 0, 0) == (255 * 1023 + 256) >> 9);
    CHECK(blend_a64(64, 7, 900) == 7 && blend_a64(0, 7, 900) == 900 && blend_a64(32, 0, 1023) == 512 && blend_avg(3, 4) == 4);

    // every plane tile's edges fit the slot's window slice, and a gathered item's slices the wave's window budget
    for (auto &s : kPlaneSizes) {
        const int tw = s[0], th = s[1], units = tw * th / 4, slots = units >= 64 ? 1 : 64 / units;
        CHECK(tw + th <= (th + 7) * (tw + 8) && slots * (th + 7) * (tw + 8) <= pred_plan::kWinCap);
    }

    // the tables: "S w h mode" then h rows; "W w h index ss" then the plane's rows
    for (auto &s : kPlaneSizes)
        for (int mode = 0; mode < kModes; mode++) {
            printf("S %d %d %d\n", s[0], s[1], mode);
            for (int r = 0; r < s[1]; r++) {
                for (int c = 0; c < s[0]; c++) printf("%d ", smooth_mask(mode, log2_of(s[0]), log2_of(s[1]), r, c));
                printf("\n");
            }
        }
    for (auto &s : kSizes)
        for (int index = 0; index < 16; index++)
            for (int ss = 0; ss < 2; ss++) {
                const wedge_masks::Plan p = wedge_masks::plan(log2_of(s[0]), log2_of(s[1]), index, 0);
                printf("W %d %d %d %d\n", s[0], s[1], index, ss);
                for (int r = 0; r < (s[1] >> ss); r++) {
                    for (int c = 0; c < (s[0] >> ss); c++) printf("%d ", wedge_mask_plane(p, ss, r, c));
                    printf("\n");
                }
            }
    fprintf(stderr, "interintra_plan_check ok: 7 sizes, 10 plane sizes, 40 smooth masks, 224 wedge masks\n");
    return 0;
}
