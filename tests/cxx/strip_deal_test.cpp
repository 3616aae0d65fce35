// Host-only check of the block -> strip map of the level-1 tile kernels (ed_tile.h: strip_of_block,
// strip_decode) -- no HIP call is made.  Built and run by tests/test_host_logic.py.
#include <cstdio>
#include <vector>

#include "ed_tile.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// every tile of `nsample` volumes of tz x ty x tx tiles, in strips of `strip_tiles`, comes out exactly once
static int decode_covers(int tz, int ty, int tx, int strip_tiles, int nsample)
{
    using ed::tile::Strip;
    const int strips_x = (tx + strip_tiles - 1) / strip_tiles;
    const int nstrips = tz * ty * strips_x;
    std::vector<int> seen((size_t)nsample * tz * ty * tx, 0);
    for (int s = 0; s < nstrips * nsample; ++s) {
        Strip sp;
        ed::tile::strip_decode(sp, s, nstrips, strips_x, ty, tx, strip_tiles);
        CHECK(sp.sample >= 0 && sp.sample < nsample);
        CHECK(sp.tz >= 0 && sp.tz < tz && sp.ty >= 0 && sp.ty < ty);
        CHECK(sp.tx0 >= 0 && sp.tx0 % strip_tiles == 0);
        CHECK(sp.ntile >= 1 && sp.ntile <= strip_tiles && sp.tx0 + sp.ntile <= tx);
        for (int t = 0; t < sp.ntile; ++t)
            ++seen[(((size_t)sp.sample * tz + sp.tz) * ty + sp.ty) * tx + sp.tx0 + t];
    }
    for (int v : seen)
        CHECK(v == 1);
    return 0;
}

int main()
{
    using ed::tile::strip_of_block;
    for (int total = 1; total <= 200; ++total) {
        const int grid = 8 * ((total + 7) / 8);
        std::vector<int> seen(total, 0);
        int s;
        for (int b = 0; b < grid; ++b) {
            if (strip_of_block(b, total, s)) {
                CHECK(s >= 0 && s < total);
                ++seen[s];
            }
        }
        for (int v : seen)
            CHECK(v == 1);
        for (int b = grid; b < 2 * grid; ++b)       // a larger grid deals no strip twice
            CHECK(!strip_of_block(b, total, s));
    }
    CHECK(decode_covers(1, 1, 1, 8, 1) == 0);
    CHECK(decode_covers(3, 5, 7, 4, 1) == 0);
    CHECK(decode_covers(2, 2, 9, 2, 3) == 0);
    std::printf("ok\n");
    return 0;
}
