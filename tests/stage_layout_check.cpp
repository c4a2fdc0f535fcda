// stage_layout_check — csrc/stage_layout.h compiled alone with g++ (no HIP, no library): the growth rule of the shims'
// per-thread staging buffer and the carver that lays out the regions of one reservation.  Prints every violated check,
// exit status 1 if any.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../svt-av1_pro-anchor-v2.1.0-_amd/csrc/stage_layout.h"

static uint64_t g_state = 0x5eed57a6e0000001ull;
static uint64_t draw() { // xorshift64
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return g_state;
}

int main() {
    int fail = 0;
    // growth: at least the need, whole 4 KiB pages, monotone, and a fixed point for every need that fits
    std::vector<size_t> needs = {1, 2, 255, 256, 4095, 4096, 4097, 6143, 6144, 6145, 65536, 1000000, (size_t)1 << 31, ((size_t)1 << 32) + 5};
    for (int i = 0; i < 4000; i++) needs.push_back((size_t)(draw() % (1u << (8 + i % 24))) + 1);
    size_t prev_need = 0, prev_cap = 0;
    for (size_t k = 1; k < 20000; k++) { // monotone over a dense range
        const size_t cap = stage_grown_capacity(k);
        if (cap < prev_cap && ++fail <= 20) std::fprintf(stderr, "capacity falls from %zu (need %zu) to %zu (need %zu)\n", prev_cap, prev_need, cap, k);
        prev_need = k, prev_cap = cap;
    }
    for (size_t need : needs) {
        const size_t cap = stage_grown_capacity(need);
        if ((cap < need || cap % 4096) && ++fail <= 20) std::fprintf(stderr, "need %zu: capacity %zu\n", need, cap);
        if (stage_grown_capacity(need + 1) < cap && ++fail <= 20) std::fprintf(stderr, "need %zu: not monotone\n", need);
        // a buffer of that capacity stays as it is for every need that fits, and grows for the first that does not
        for (size_t fits : {need, cap, cap - 1, (need + cap) / 2, (size_t)1, (size_t)0})
            if (stage_capacity_for(cap, fits) != cap && ++fail <= 20) std::fprintf(stderr, "capacity %zu changes for need %zu\n", cap, fits);
        if (stage_capacity_for(cap, cap + 1) <= cap && ++fail <= 20) std::fprintf(stderr, "capacity %zu does not grow for %zu\n", cap, cap + 1);
        if (stage_capacity_for(0, need) != cap && ++fail <= 20) std::fprintf(stderr, "an empty buffer takes %zu for need %zu\n", stage_capacity_for(0, need), need);
    }
    // carving: 256-aligned, from 0, disjoint, in order, covered by the end
    long lists = 0;
    for (int t = 0; t < 3000; t++) {
        Carver    c;
        const int n = 1 + (int)(draw() % 12);
        size_t    end_prev = 0;
        for (int i = 0; i < n; i++) {
            const uint64_t r = draw();
            const size_t   bytes = r % 5 == 0 ? 0 : r % 5 == 1 ? 1 : (size_t)((r >> 8) % (1u << (4 + (r >> 40) % 20)));
            const size_t   o = c(bytes);
            if (i == 0 && o != 0) fail++, std::fprintf(stderr, "list %d: the first region starts at %zu\n", t, o);
            if ((o % kStageAlign || o < end_prev || c.off < o + bytes || c.off % kStageAlign) && ++fail <= 20)
                std::fprintf(stderr, "list %d region %d: offset %zu, %zu bytes, previous end %zu, carver end %zu\n", t, i, o, bytes, end_prev, c.off);
            end_prev = o + bytes;
        }
        lists++;
    }
    if (kStageAlign != 256) fail++, std::fprintf(stderr, "the alignment is %zu\n", kStageAlign);
    if (fail) std::fprintf(stderr, "stage_layout_check: %d checks failed\n", fail);
    else std::printf("stage_layout_check ok: %zu needs, %ld size lists\n", needs.size(), lists);
    return fail ? 1 : 0;
}
