// A stand-alone run of the overview builder's host code (csrc/ortho_overview.hpp, csrc/host/ortho_overview.cpp) for the
// address and undefined-behaviour sanitizers.  Part 1: progress::feed over random rasters and band partitions, with and
// without fused blocks - every row of every level written exactly once, only from source rows that are complete and (level
// 1) inside the band or the pending row, fused blocks aligned and inside the band.  Part 2: the CPU route through the C ABI,
// both kinds, every band in a heap block of exactly its size so that a read past either end is caught, random partitions
// against one feed of the whole raster.  Host code only; from the repository root:
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude scripts/ortho_overviews_sanitize.cpp opencalibration_amd/csrc/host/ortho_overview.cpp -o ortho_overviews_sanitize
//   ./ortho_overviews_sanitize
//
// The device route is not linked: its entry points that ortho_overview.cpp names are stubs here and never called.
#include "../include/oc_host.h"
#include "../opencalibration_amd/csrc/ortho_overview.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

extern "C"
{
int ochip_ortho_overviews_create(ochip_ctx *, int, int64_t, int64_t, void *const *, int, ochip_ortho_overviews **)
{
    std::abort();
}
int ochip_ortho_overviews_feed(ochip_ortho_overviews *, int64_t, int64_t, const void *)
{
    std::abort();
}
int64_t ochip_ortho_overviews_complete_rows(const ochip_ortho_overviews *, int)
{
    std::abort();
}
int ochip_ortho_overviews_finish(ochip_ortho_overviews *)
{
    std::abort();
}
void ochip_ortho_overviews_destroy(ochip_ortho_overviews *o)
{
    if (o)
        std::abort();
}
const char *ochip_last_error(const ochip_ctx *)
{
    return "";
}
}

using namespace ochip_ov;

static int check_plans()
{
    std::mt19937 rng(5);
    long checked = 0;
    for (int trial = 0; trial < 3000; trial++)
    {
        const int64_t w = 1 + rng() % 200, h = 1 + rng() % 400;
        for (int fused = 0; fused < 2; fused++)
        {
            progress P;
            P.reset(w, h);
            std::vector<std::vector<int>> written(P.levels + 1);
            for (int k = 1; k <= P.levels; k++)
                written[k].assign(P.level_h(k), 0);
            int64_t row0 = 0;
            bool pending = false;
            while (row0 < h)
            {
                int64_t rows = 1 + rng() % (trial % 3 == 0 ? 200 : 70);
                if (rows > h - row0)
                    rows = h - row0;
                std::vector<step> steps;
                std::string e = P.feed(row0, rows, fused, &steps);
                if (!e.empty()) { printf("refused %s\n", e.c_str()); return 1; }
                auto src_ok = [&](int k, int64_t r, bool top) {
                    // the source rows of row r of level k
                    for (int64_t s = 2 * r; s <= 2 * r + 1 && s < P.level_h(k - 1); s++)
                    {
                        if (k == 1)
                        {
                            if (top && s == 2 * r) { if (!pending || s != row0 - 1) return false; }
                            else if (s < row0 || s >= row0 + rows) return false;
                        }
                        else if (written[k - 1][s] != 1) return false;
                    }
                    return true;
                };
                for (const step &s : steps)
                {
                    if (s.what == step::KEEP) { if (s.r0 != row0 + rows - 1) return 2; pending = true; continue; }
                    if (s.what == step::PLAIN)
                    {
                        for (int64_t r = s.r0; r < s.r1; r++)
                        {
                            if (r < 0 || r >= P.level_h(s.level) || !src_ok(s.level, r, s.top_pending && r == s.r0)) { printf("bad plain w %ld h %ld level %d row %ld\n", (long)w, (long)h, s.level, (long)r); return 3; }
                            written[s.level][r]++;
                        }
                        if (s.top_pending) pending = false;
                    }
                    else
                    {
                        if (s.r0 % 64 || (s.r1 % 64 && s.r1 != h) || s.r0 < row0 || s.r1 > row0 + rows || s.r1 <= s.r0) return 4;
                        const int fd = P.levels < 6 ? P.levels : 6;
                        for (int k = 1; k <= fd; k++)
                            for (int64_t r = s.r0 >> k; r < (s.r1 == h ? P.level_h(k) : s.r1 >> k); r++)
                                written[k][r]++;
                    }
                }
                for (int k = 1; k <= P.levels; k++)
                    for (int64_t r = 0; r < P.level_h(k); r++)
                        if (written[k][r] != (r < P.done[k] ? 1 : 0)) { printf("w %ld h %ld fused %d level %d row %ld written %d done %ld\n", (long)w, (long)h, fused, k, (long)r, written[k][r], (long)P.done[k]); return 5; }
                row0 += rows;
                checked++;
            }
            if (!P.finish().empty()) return 6;
            for (int k = 1; k <= P.levels; k++)
                if (P.done[k] != P.level_h(k)) return 7;
        }
    }
    printf("plans ok: %ld feeds\n", checked);
    return 0;
}

// the levels of a raster fed in bands of at most max_rows random rows (0: one feed), each band in its own exact heap block
static int build(int kind, int64_t w, int64_t h, const uint32_t *level0, int64_t max_rows, std::mt19937 &rng,
                 std::vector<std::unique_ptr<uint32_t[]>> *levels)
{
    int64_t sizes[2 * MAX_LEVELS];
    const int n = och_ortho_overviews_levels(w, h, sizes);
    std::vector<void *> ptrs;
    levels->clear();
    for (int k = 0; k < n; k++)
    {
        levels->emplace_back(new uint32_t[(size_t)(sizes[2 * k] * sizes[2 * k + 1])]);
        ptrs.push_back(levels->back().get());
    }
    och_ortho_overviews *o = nullptr;
    if (och_ortho_overviews_create(nullptr, kind, w, h, ptrs.data(), 0, &o) != 0)
        return 1;
    for (int64_t row0 = 0; row0 < h;)
    {
        int64_t rows = max_rows ? 1 + (int64_t)(rng() % max_rows) : h;
        rows = rows > h - row0 ? h - row0 : rows;
        std::unique_ptr<uint32_t[]> band(new uint32_t[(size_t)(rows * w)]);
        std::memcpy(band.get(), level0 + row0 * w, (size_t)(rows * w) * 4);
        if (och_ortho_overviews_feed(o, row0, rows, band.get()) != 0)
            return 2;
        row0 += rows;
    }
    if (och_ortho_overviews_finish(o) != 0)
        return 3;
    for (int k = 0; k < n; k++)
        if (och_ortho_overviews_complete_rows(o, k + 1) != sizes[2 * k])
            return 4;
    och_ortho_overviews_destroy(o);
    return 0;
}

int main()
{
    if (int rc = check_plans())
    {
        printf("plan check failed: %d\n", rc);
        return 1;
    }
    std::mt19937 rng(11);
    const int64_t shapes[][2] = {{1, 1}, {2, 9}, {3, 3}, {64, 64}, {65, 65}, {130, 67}, {129, 200}, {1000, 5}, {1, 300}, {517, 333}};
    for (const auto &shape : shapes)
        for (int kind = 0; kind < 2; kind++)
        {
            const int64_t w = shape[0], h = shape[1];
            std::unique_ptr<uint32_t[]> level0(new uint32_t[(size_t)(w * h)]);
            for (int64_t i = 0; i < w * h; i++)
            {
                if (kind == OCHIP_OVERVIEW_RGBA8)
                    level0[i] = (uint32_t)rng() & (rng() % 3 ? 0xFFFFFFFFu : 0x00FFFFFFu);
                else
                {
                    const float f = rng() % 4 ? (float)(rng() % 100000) * 0.37f - 500.0f : NAN;
                    std::memcpy(&level0[i], &f, 4);
                }
            }
            std::vector<std::unique_ptr<uint32_t[]>> whole, banded;
            if (int rc = build(kind, w, h, level0.get(), 0, rng, &whole))
            {
                printf("%lld x %lld kind %d: whole feed failed (%d): %s\n", (long long)w, (long long)h, kind, rc, och_ortho_overviews_last_error());
                return 1;
            }
            for (int64_t max_rows : {1, 3, 64, 150})
            {
                if (int rc = build(kind, w, h, level0.get(), max_rows, rng, &banded))
                {
                    printf("%lld x %lld kind %d: banded feed failed (%d): %s\n", (long long)w, (long long)h, kind, rc, och_ortho_overviews_last_error());
                    return 1;
                }
                for (size_t k = 0; k < whole.size(); k++)
                    if (std::memcmp(whole[k].get(), banded[k].get(), (size_t)(level_extent(w, (int)k + 1) * level_extent(h, (int)k + 1)) * 4) != 0)
                    {
                        printf("%lld x %lld kind %d: level %zu differs between one feed and bands of up to %lld rows\n", (long long)w, (long long)h, kind, k + 1, (long long)max_rows);
                        return 1;
                    }
            }
        }
    printf("CPU route ok\n");
    return 0;
}
