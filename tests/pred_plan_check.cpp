// pred_plan_check — csrc/pred_plan.h compiled alone with g++ (no HIP, no library): the block predictors' size rule, the
// wave items of the tile kernels and of the warp kernel against the LDS budget and an exact cover of every block, the
// plane checks' boundary cases, the MV clamp against the formula written out here, and the metadata layout.  Prints every
// violated check, exit status 1 if any.
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "../svt-av1_pro-anchor-v2.1.0-_amd/csrc/pred_plan.h"

using namespace pred_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond) && ++g_fail <= 30) std::fprintf(stderr, __VA_ARGS__);   \
    } while (0)

// compound_cases.SIZES
static const int kSizes[17][2] = {{8, 8}, {8, 16}, {16, 8}, {8, 32}, {32, 8}, {16, 16}, {16, 32}, {32, 16}, {16, 64}, {64, 16},
                                  {32, 32}, {32, 64}, {64, 32}, {64, 64}, {64, 128}, {128, 64}, {128, 128}};
// compound_cases.batch_cases()[0]: 23 blocks that tile 256 x 192 (x, y, w, h)
static const int kTiling[23][4] = {{0, 0, 128, 128}, {128, 0, 128, 64}, {128, 64, 64, 128}, {192, 64, 64, 64}, {192, 128, 64, 32},
    {192, 160, 32, 32}, {224, 160, 32, 16}, {224, 176, 16, 16}, {240, 176, 8, 16}, {248, 176, 8, 8}, {248, 184, 8, 8}, {0, 128, 32, 64},
    {32, 128, 64, 32}, {32, 160, 64, 16}, {32, 176, 32, 8}, {32, 184, 32, 8}, {64, 176, 16, 16}, {80, 176, 16, 8}, {80, 184, 16, 8},
    {96, 128, 16, 64}, {112, 128, 16, 32}, {112, 160, 8, 32}, {120, 160, 8, 32}};

// one item against the slot cap and the LDS budget; returns its capacity in slots
static int check_item(const CompItem &it) {
    const int tw = 1 << it.tw_log2, th = 1 << it.th_log2, units = tw * th / 4, cap = units >= 64 ? 1 : 64 / units;
    CHECK(it.nslots >= 1 && it.nslots <= cap && it.nslots <= kMaxSlots, "item %dx%d: %d slots, cap %d\n", tw, th, it.nslots, cap);
    CHECK(it.nslots * (th + 7) * (tw + 8) <= kWinCap, "item %dx%d x %d: window past kWinCap\n", tw, th, it.nslots);
    CHECK(it.nslots * (th + 7) * tw <= kImCap, "item %dx%d x %d: intermediate past kImCap\n", tw, th, it.nslots);
    CHECK(tw <= kTile && th <= kTile && tw >= 4 && th >= 4, "item %dx%d: tile outside 4 .. %d\n", tw, th, kTile);
    return cap;
}

int main() {
    long n_items = 0, n_warp = 0, n_mv = 0;
    // block_size_ok: exactly the 17 sizes
    int accepted = 0;
    for (int wl = 3; wl <= 7; wl++)
        for (int hl = 3; hl <= 7; hl++) {
            bool listed = false;
            for (auto &s : kSizes) listed |= s[0] == (1 << wl) && s[1] == (1 << hl);
            CHECK(block_size_ok(wl, hl) == listed, "block_size_ok(%d, %d) is %d\n", wl, hl, (int)block_size_ok(wl, hl));
            accepted += block_size_ok(wl, hl);
        }
    CHECK(accepted == 17 && !block_size_ok(2, 3) && !block_size_ok(3, 2) && !block_size_ok(8, 7), "%d sizes accepted\n", accepted);

    // ItemBuilder::add_plane: every size, every plane, alone
    for (auto &s : kSizes)
        for (int p = 0; p < 3; p++) {
            const int   wl = log2_of(s[0]), hl = log2_of(s[1]), pw = s[0] >> (p > 0), ph = s[1] >> (p > 0);
            ItemBuilder ib;
            ib.add_plane(7, p, wl, hl);
            std::vector<int> hits((size_t)pw * ph, 0);
            for (const CompItem &it : ib.items) {
                check_item(it), n_items++;
                for (int k = 0; k < it.nslots; k++) {
                    const CompSlot &sl = it.slot[k];
                    CHECK(sl.blk == 7 && sl.plane == p, "%dx%d plane %d: a slot of block %u plane %d\n", s[0], s[1], p, sl.blk, sl.plane);
                    for (int y = 0; y < (1 << it.th_log2); y++)
                        for (int x = 0; x < (1 << it.tw_log2); x++) {
                            const int gx = sl.ox + x, gy = sl.oy + y;
                            CHECK(gx < pw && gy < ph, "%dx%d plane %d: sample (%d, %d) outside\n", s[0], s[1], p, gx, gy);
                            if (gx < pw && gy < ph) hits[(size_t)gy * pw + gx]++;
                        }
                }
            }
            for (int v : hits) CHECK(v == 1, "%dx%d plane %d: a sample in %d tiles\n", s[0], s[1], p, v);
        }
    // the fixture's tiling with chroma: every (block, plane, tile) once, only a shape's last item under-filled
    {
        ItemBuilder ib;
        std::map<std::tuple<int, int, int, int>, int> want, got;
        for (int i = 0; i < 23; i++)
            for (int p = 0; p < 3; p++) {
                const int wl = log2_of(kTiling[i][2]), hl = log2_of(kTiling[i][3]);
                CHECK(check_block_rect(kTiling[i][0], kTiling[i][1], wl, hl, 4, 256, 192), "tiling block %d refused\n", i);
                ib.add_plane((uint32_t)i, p, wl, hl);
                const int pw = kTiling[i][2] >> (p > 0), ph = kTiling[i][3] >> (p > 0), tw = pw < 32 ? pw : 32, th = ph < 32 ? ph : 32;
                for (int oy = 0; oy < ph; oy += th)
                    for (int ox = 0; ox < pw; ox += tw) want[{i, p, ox, oy}]++;
            }
        std::map<std::pair<int, int>, int> last_of_shape;
        for (size_t k = 0; k < ib.items.size(); k++) last_of_shape[{ib.items[k].tw_log2, ib.items[k].th_log2}] = (int)k;
        for (size_t k = 0; k < ib.items.size(); k++) {
            const CompItem &it = ib.items[k];
            const int       cap = check_item(it);
            n_items++;
            const bool last = last_of_shape[std::make_pair((int)it.tw_log2, (int)it.th_log2)] == (int)k;
            CHECK(it.nslots == cap || last, "item %zu is under-filled (%d of %d) and not its shape's last\n", k, it.nslots, cap);
            for (int s = 0; s < it.nslots; s++) got[{(int)it.slot[s].blk, it.slot[s].plane, it.slot[s].ox, it.slot[s].oy}]++;
        }
        CHECK(want == got, "the tiling's tiles: %zu wanted, %zu in the items\n", want.size(), got.size());
        for (auto &kv : got) CHECK(kv.second == 1, "a tile occurs %d times\n", kv.second);
    }

    // warp_items
    for (auto &s : kSizes)
        for (int chroma = 0; chroma < 2; chroma++) {
            std::vector<WarpItem> items;
            warp_items(3, log2_of(s[0]), log2_of(s[1]), chroma != 0, [&](const WarpItem &it) { items.push_back(it); });
            const int                         np = chroma && s[0] >= 16 && s[1] >= 16 ? 3 : 1;
            std::map<std::tuple<int, int, int>, int> units;
            for (const WarpItem &it : items) {
                int gw, n;
                warp_shape_decode(it.shape, &gw, &n);
                n_warp++;
                CHECK(it.blk == 3 && it.plane < np && n >= 1 && n <= 4 && (gw == 1 || gw == 2), "%dx%d: item plane %d gw %d n %d\n", s[0], s[1], it.plane, gw, n);
                for (int v = 0; v < n; v++) units[{it.plane, it.ux + v % gw, it.uy + v / gw}]++;
            }
            size_t expect = 0;
            for (int p = 0; p < np; p++) {
                const int uw = (s[0] >> (p > 0)) / 8, uh = (s[1] >> (p > 0)) / 8;
                expect += (size_t)uw * uh;
                for (int uy = 0; uy < uh; uy++)
                    for (int ux = 0; ux < uw; ux++) CHECK((units[{p, ux, uy}] == 1), "%dx%d chroma %d: unit (%d, %d, %d) in %d waves\n", s[0], s[1], chroma, p, ux, uy, units[{p, ux, uy}]);
            }
            CHECK(units.size() == expect, "%dx%d chroma %d: %zu units, %zu expected\n", s[0], s[1], chroma, units.size(), expect);
        }
    for (int gw = 1; gw <= 2; gw++)
        for (int n = 1; n <= 4; n++) {
            int g2, n2;
            warp_shape_decode(warp_shape_encode(gw, n), &g2, &n2);
            CHECK(g2 == gw && n2 == n, "shape (%d, %d) decodes to (%d, %d)\n", gw, n, g2, n2);
        }

    // check_planes: each boundary case flips the result on its own (width 64, border 16, 10-bit)
    {
        alignas(16) static uint16_t mem[64];
        const int      width = 64, border = 16;
        SvtGpuTfPlanes ref = {{mem, mem, mem}, {width + 2 * border, (width >> 1) + 2 * (border >> 1), (width >> 1) + 2 * (border >> 1)}};
        SvtGpuTfPlanes pred = {{mem, mem, mem}, {64, 32, 32}};
        auto           ok = [&](const SvtGpuTfPlanes &r, const SvtGpuTfPlanes &p, int bd, int nplanes) { return check_planes(&r, 1, &p, width, border, bd, nplanes); };
        CHECK(ok(ref, pred, 10, 3) && ok(ref, pred, 8, 3), "the exact strides are refused\n");
        for (int p = 0; p < 3; p++) {
            SvtGpuTfPlanes r = ref, q = pred;
            r.stride[p]--;
            CHECK(!ok(r, pred, 10, 3), "plane %d: a reference stride one short is accepted\n", p);
            q.stride[p] += 4; // 8 bytes at 16 bits
            CHECK(!ok(ref, q, 10, 3), "plane %d: a pred stride of %d bytes is accepted\n", p, q.stride[p] * 2);
            q = pred, q.plane[p] = (uint8_t *)mem + 8;
            CHECK(!ok(ref, q, 10, 3), "plane %d: a pred pointer off by 8 is accepted\n", p);
            r = ref, r.plane[p] = (uint8_t *)mem + 1;
            CHECK(!ok(r, pred, 10, 3) && ok(r, pred, 8, 3), "plane %d: a reference pointer off by 1 (refused at 16 bits only)\n", p);
        }
        for (int p = 1; p < 3; p++) {
            SvtGpuTfPlanes r = ref, q = pred;
            r.plane[p] = nullptr, q.plane[p] = nullptr;
            CHECK(!ok(r, pred, 10, 3) && !ok(ref, q, 10, 3) && ok(r, q, 10, 1), "plane %d: a null chroma plane\n", p);
        }
        CHECK(check_planes(&ref, 1, &pred, width, 0, 10, 3) && !check_planes(&ref, 1, &pred, width, border + 2, 10, 3), "the border term\n");
    }

    // clamped_mv against the formula written out here (clamp_mv_to_umv_border_sb, 1/16 sample of the plane)
    {
        // +-INT16 / 2 wrap in the first cast (times 2 at luma), +-INT16 / 8 do not: both casts bear load
        const int W = 256, H = 192, mvs[7] = {INT16_MIN / 8, INT16_MAX / 8, 0, 1, -1, INT16_MIN / 2 - 3, INT16_MAX / 2 + 3};
        for (int b : {8, 128})
            for (int corner = 0; corner < 4; corner++)
                for (int ss = 0; ss < 2; ss++)
                    for (int mv : mvs)
                        for (int dim = 0; dim < 2; dim++) {
                            const int size = dim ? H : W, org = (corner >> dim) & 1 ? size - b : 0;
                            const int scaled = ss ? mv : mv * 2; // 1/8 luma -> 1/16 of the plane
                            int       q = (int16_t)scaled;
                            const int to_edge_lo = ss ? -(org * 8) : -(org * 16), to_edge_hi = ss ? (size - b - org) * 8 : (size - b - org) * 16;
                            const int margin = (4 + (ss ? b / 2 : b)) * 16;
                            if (q < to_edge_lo - margin) q = to_edge_lo - margin;
                            if (q > to_edge_hi + margin - 16) q = to_edge_hi + margin - 16;
                            q = (int16_t)q;
                            const int got = clamped_mv(mv, org, b, size, ss);
                            CHECK(got == q, "clamped_mv(%d, %d, %d, %d, %d) = %d, expected %d\n", mv, org, b, size, ss, got, q);
                            n_mv++;
                        }
    }

    // MetaLayout
    int n_lay = 0;
    for (size_t n_refs : {0, 1, 26})
        for (size_t n_blocks : {0, 1, 3})
            for (size_t bsz : {32, 76})
                for (size_t n_it : {0, 1, 5})
                    for (size_t isz : {8, 144}) {
                        const MetaLayout l(n_refs, n_blocks, bsz, n_it, isz);
                        CHECK(l.o_blk % 16 == 0 && l.o_item % 16 == 0, "layout: offsets %zu, %zu\n", l.o_blk, l.o_item);
                        CHECK(l.ref_bytes == n_refs * sizeof(SvtGpuTfPlanes) && l.blk_bytes == n_blocks * bsz && l.item_bytes == n_it * isz, "layout: sizes\n");
                        CHECK(l.ref_bytes <= l.o_blk && l.o_blk + l.blk_bytes <= l.o_item && l.o_item + l.item_bytes == l.total, "layout: regions overlap\n");
                        n_lay++;
                    }
    CHECK(batch_args_ok(&n_lay, &n_lay, 0, nullptr, 0, 8, &n_lay) && !batch_args_ok(&n_lay, &n_lay, 0, nullptr, 0, 8, &n_lay, 0, -1) && kMaxRefs == 26 && kWaveLds == kWinCap + kImCap && dist_wtd_ok(0, 0, 0) && dist_wtd_ok(1, 9, 7) && !dist_wtd_ok(1, 9, 8) && !dist_wtd_ok(2, 9, 7),
          "constants or dist_wtd_ok\n");
    CHECK(size_ok(2, 2) && !size_ok(2, 4) && size_ok(128, 4) && !size_ok(256, 2) && !size_ok(24, 2) && rounds_ok(3, 7) && !rounds_ok(7, 8) && !rounds_ok(-1, 3) && align16(17) == 32, "predicates\n");

    if (g_fail) std::fprintf(stderr, "pred_plan_check: %d checks failed\n", g_fail);
    else std::printf("pred_plan_check ok: 17 sizes, %ld tile items, %ld warp items, %ld clamped MVs, %d layouts\n", n_items, n_warp, n_mv, n_lay);
    return g_fail ? 1 : 0;
}
