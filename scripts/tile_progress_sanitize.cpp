// A stand-alone run of the tile-progress host code (csrc/ortho_tile_thumbs.hpp, csrc/host/ortho_tile_thumbs.cpp) for the
// address and undefined-behaviour sanitizers.  Every input array - the layers' BGRA, their weights, the blended RGBA - sits in
// a heap block of exactly its size, so that a read past either end is a report; the records and the slots the object returns
// are compared with the reference's two loops (src/ortho/ortho.cpp:1553-1614, 1962-2011) written out here once more.  The
// cases: the shapes, layer counts and contents of tests/test_tile_progress_host.py, rasters fed in bands, and the refusals.
// Host code only; from the repository root:
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude scripts/tile_progress_sanitize.cpp opencalibration_amd/csrc/host/ortho_tile_thumbs.cpp -o tile_progress_sanitize
//   ./tile_progress_sanitize
//
// The device route is not linked: its entry points that ortho_tile_thumbs.cpp names are stubs here and never called.
#include "../include/oc_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

extern "C"
{
int ochip_ortho_tile_thumbs_enqueue(ochip_ctx *, int, int32_t, int64_t, int32_t, int32_t, int, const uint8_t *, const float *,
                                    ochip_tile_thumbs_job **)
{
    std::abort();
}
int ochip_ortho_tile_thumbs_wait(ochip_tile_thumbs_job *, const uint8_t **, uint64_t *)
{
    std::abort();
}
void ochip_ortho_tile_thumbs_release(ochip_tile_thumbs_job *j)
{
    if (j)
        std::abort();
}
const char *ochip_last_error(const ochip_ctx *)
{
    return "";
}
}

namespace
{

int failures = 0;

void expect(bool ok, const char *what, long a = 0, long b = 0, long c = 0)
{
    if (!ok)
    {
        std::fprintf(stderr, "FAILED: %s (%ld, %ld, %ld): %s\n", what, a, b, c, och_tile_progress_last_error());
        failures++;
    }
}

const char *const CONTENTS[] = {"all_invalid", "only_layer_1", "equal_weights", "heavier_upper", "weight_zero", "nan_alone",
                                "nan_beside_finite", "weight_minus_half", "mixed"};

// one band's inputs, each in a block of exactly its size
struct band_data
{
    int L;
    int64_t rows, cols;
    std::unique_ptr<uint8_t[]> bgra, rgba;
    std::unique_ptr<float[]> weight;
};

band_data make(int content, int L, int64_t rows, int64_t cols, std::mt19937 &rng)
{
    band_data d{L, rows, cols, nullptr, nullptr, nullptr};
    const size_t plane = (size_t)(rows * cols);
    d.bgra.reset(new uint8_t[(size_t)L * plane * 4]);
    d.weight.reset(new float[(size_t)L * plane]);
    d.rgba.reset(new uint8_t[plane * 4]);
    const float picks[] = {NAN, -0.5f, -0.0f, 0.0f, 0.0005f, 1.0f, 1.0f, 2.5f, INFINITY};
    const uint8_t alphas[] = {0, 0, 1, 255};
    for (int l = 0; l < L; l++)
        for (size_t i = 0; i < plane; i++)
        {
            uint8_t *px = &d.bgra[((size_t)l * plane + i) * 4];
            for (int c = 0; c < 4; c++)
                px[c] = (uint8_t)(1 + rng() % 255);
            float w = 0.001f + (float)(rng() % 2000) * 0.001f;
            switch (content)
            {
            case 0: px[3] = 0; break;
            case 1: if (l != std::min(1, L - 1) || rng() % 2) px[3] = 0; break;
            case 2: if (l == 0 || l == L - 1) w = 3.0f; break;
            case 3: w += (float)l * 2.0f; break;
            case 4: w = 0.0f; break;
            case 5: w = NAN; break;
            case 6: if ((l == 0 && i % 2 == 0) || (l == L - 1 && i % 2 == 1)) w = NAN; break;
            case 7: w = -0.5f; break;
            default: px[3] = alphas[rng() % 4], w = picks[rng() % 9]; break;
            }
            d.weight[(size_t)l * plane + i] = w;
        }
    for (size_t i = 0; i < plane; i++)
    {
        uint8_t *px = &d.rgba[i * 4];
        const uint8_t grey = (i / 8) % 2 ? 64 : 128;
        const int kind = content % 3; // the blend's checkerboard (alpha 0, grey), alpha 1, mixed
        for (int c = 0; c < 3; c++)
            px[c] = kind == 0 ? grey : (uint8_t)(1 + rng() % 255);
        px[3] = kind == 0 ? 0 : kind == 1 ? 1 : alphas[rng() % 4];
    }
    return d;
}

// the reference's loops over one tile: the slot's expected bytes (the thumbnail densely, zeros behind it)
void expected_slot(const band_data &d, int pass, int64_t x_off, int64_t y_off, int tw, int th, size_t slot_pixels, uint8_t *slot, int *dims)
{
    const int scale = std::max(1, (std::max(tw, th) + 127) / 128);
    const int thumb_w = (tw + scale - 1) / scale, thumb_h = (th + scale - 1) / scale;
    dims[0] = scale, dims[1] = thumb_w, dims[2] = thumb_h;
    std::memset(slot, 0, slot_pixels * 4);
    const size_t plane = (size_t)(d.rows * d.cols);
    for (int ty = 0; ty < thumb_h; ty++)
        for (int tx = 0; tx < thumb_w; tx++)
        {
            const int src_row = std::min(ty * scale, th - 1), src_col = std::min(tx * scale, tw - 1);
            const size_t at = (size_t)(y_off + src_row) * (size_t)d.cols + (size_t)(x_off + src_col);
            uint8_t *out = slot + ((size_t)ty * thumb_w + tx) * 4;
            if (pass == 1)
            {
                float best_weight = -1.f;
                uint8_t best_color[3] = {0, 0, 0};
                for (int layer = 0; layer < d.L; layer++)
                {
                    const uint8_t *sample = &d.bgra[((size_t)layer * plane + at) * 4];
                    const float weight = d.weight[(size_t)layer * plane + at];
                    if (sample[3] > 0 && weight > best_weight)
                    {
                        best_weight = weight;
                        std::memcpy(best_color, sample, 3);
                    }
                }
                out[3] = 255 * 20 / 100;
                if (best_weight >= 0.f)
                {
                    std::memcpy(out, best_color, 3);
                    out[3] = 255;
                }
            }
            else if (d.rgba[at * 4 + 3] > 0)
            {
                out[0] = d.rgba[at * 4 + 2], out[1] = d.rgba[at * 4 + 1], out[2] = d.rgba[at * 4 + 0];
                out[3] = 255;
            }
        }
}

// a raster of `height` rows fed in bands of band_tile_rows tile rows, both passes, every band in blocks of its own
void run_raster(int content, int L, int64_t cols, int64_t height, int T, int band_tile_rows, std::mt19937 &rng)
{
    const double plan8[8] = {(double)cols, (double)height, 0.125, -3.5, 0, 0, 2.25, 40.0};
    och_tile_progress *p = nullptr;
    expect(och_tile_progress_create(nullptr, plan8, T, L, &p) == 0, "create", (long)cols, (long)height, T);
    if (!p)
        return;
    const int64_t tiles_x = (cols + T - 1) / T, tiles_y = (height + T - 1) / T;
    const size_t side = (size_t)std::min(T, 128), slot_pixels = side * side;
    const int64_t band_rows = (int64_t)band_tile_rows * T;
    for (int64_t row0 = 0; row0 < height; row0 += band_rows)
    {
        const int64_t rows = std::min(band_rows, height - row0);
        const band_data d = make(content, L, rows, cols, rng);
        expect(och_tile_progress_feed(p, 1, row0, rows, 0, d.bgra.get(), d.weight.get()) == 0, "feed pass 1", (long)row0, (long)rows, T);
        expect(och_tile_progress_feed(p, 2, row0, rows, 0, d.rgba.get(), nullptr) == 0, "feed pass 2", (long)row0, (long)rows, T);
        expect(och_tile_progress_pending(p) == 2, "two bands pending");
        for (int pass = 1; pass <= 2; pass++)
        {
            uint64_t n = 0;
            expect(och_tile_progress_collect(p, nullptr, nullptr, 0, &n) == 0, "tile count");
            const int64_t band_tiles = tiles_x * ((rows + T - 1) / T);
            expect((int64_t)n == band_tiles, "tiles of the band", (long)n, (long)band_tiles);
            std::unique_ptr<och_tile_update[]> updates(new och_tile_update[n]);
            std::unique_ptr<uint8_t[]> thumbs(new uint8_t[n * slot_pixels * 4]);
            std::unique_ptr<uint8_t[]> want(new uint8_t[slot_pixels * 4]);
            expect(och_tile_progress_collect(p, updates.get(), thumbs.get(), n, &n) == 0, "collect");
            for (int64_t t = 0; t < band_tiles; t++)
            {
                const int64_t tx = t % tiles_x, ty = t / tiles_x;
                const int tw = (int)std::min<int64_t>(T, cols - tx * T), th = (int)std::min<int64_t>(T, rows - ty * T);
                int dims[3];
                expected_slot(d, pass, tx * T, ty * T, tw, th, slot_pixels, want.get(), dims);
                expect(std::memcmp(want.get(), thumbs.get() + (size_t)t * slot_pixels * 4, slot_pixels * 4) == 0, "slot", (long)t, pass, content);
                const och_tile_update &u = updates[t];
                expect(u.pixel_x == tx * T && u.pixel_y == row0 + ty * T && u.pixel_w == tw && u.pixel_h == th &&
                           u.total_output_width == cols && u.total_output_height == height &&
                           u.tile_index == (row0 / T + ty) * tiles_x + tx + 1 && u.total_tiles == tiles_x * tiles_y &&
                           u.scale == dims[0] && u.thumb_w == dims[1] && u.thumb_h == dims[2] && u.pass == pass &&
                           u.bounds_min_x == -3.5 && u.bounds_max_y == 2.25 && u.meters_per_pixel == 0.125,
                       "record", (long)t, pass, T);
            }
        }
    }
    expect(och_tile_progress_pending(p) == 0, "nothing pending");
    och_tile_progress_destroy(p);
}

void refusals()
{
    const double plan8[8] = {70, 40, 0.125, -3.5, 0, 0, 2.25, 40.0};
    och_tile_progress *p = nullptr;
    expect(och_tile_progress_create(nullptr, plan8, 0, 2, &p) != 0 && !p, "tile_size 0");
    expect(och_tile_progress_create(nullptr, plan8, 4097, 2, &p) != 0 && !p, "tile_size 4097");
    expect(och_tile_progress_create(nullptr, plan8, 32, 0, &p) != 0 && !p, "no layers");
    expect(och_tile_progress_create(nullptr, plan8, 32, 9, &p) != 0 && !p, "nine layers");
    expect(och_tile_progress_create(nullptr, nullptr, 32, 2, &p) != 0 && !p, "no plan");
    const double empty[8] = {0, 40, 0.125, 0, 0, 0, 0, 0};
    expect(och_tile_progress_create(nullptr, empty, 32, 2, &p) != 0 && !p, "no columns");
    expect(och_tile_progress_create(nullptr, plan8, 32, 2, &p) == 0 && p, "create");
    std::mt19937 rng(3);
    const band_data d = make(8, 2, 32, 70, rng), last = make(8, 2, 8, 70, rng);
    expect(och_tile_progress_feed(nullptr, 2, 0, 32, 0, d.rgba.get(), nullptr) != 0, "no object");
    expect(och_tile_progress_feed(p, 0, 0, 32, 0, d.rgba.get(), nullptr) != 0, "pass 0");
    expect(och_tile_progress_feed(p, 3, 0, 32, 0, d.rgba.get(), nullptr) != 0, "pass 3");
    expect(och_tile_progress_feed(p, 1, 0, 32, 0, d.bgra.get(), nullptr) != 0, "pass 1 without weights");
    expect(och_tile_progress_feed(p, 2, 0, 32, 0, nullptr, nullptr) != 0, "no pixels");
    expect(och_tile_progress_feed(p, 2, 0, 32, 1, d.rgba.get(), nullptr) != 0, "device inputs without a context");
    expect(och_tile_progress_feed(p, 2, 0, 0, 0, d.rgba.get(), nullptr) != 0, "no rows");
    expect(och_tile_progress_feed(p, 2, 0, -4, 0, d.rgba.get(), nullptr) != 0, "negative rows");
    expect(och_tile_progress_feed(p, 2, 16, 16, 0, d.rgba.get(), nullptr) != 0, "off the tile rows");
    expect(och_tile_progress_feed(p, 2, 0, 20, 0, d.rgba.get(), nullptr) != 0, "a part of a tile row");
    expect(och_tile_progress_feed(p, 2, 32, 8, 0, last.rgba.get(), nullptr) != 0, "a gap");
    expect(och_tile_progress_feed(p, 2, 32, 32, 0, d.rgba.get(), nullptr) != 0, "beyond the raster");
    expect(och_tile_progress_pending(p) == 0, "refused feeds change nothing");
    expect(och_tile_progress_feed(p, 2, 0, 32, 0, d.rgba.get(), nullptr) == 0, "first band");
    expect(och_tile_progress_feed(p, 2, 0, 32, 0, d.rgba.get(), nullptr) != 0, "the same band again");
    expect(och_tile_progress_feed(p, 2, 32, 8, 0, last.rgba.get(), nullptr) == 0, "last band");
    expect(och_tile_progress_seek(p, 1, 32) == 0 && och_tile_progress_seek(p, 1, 16) != 0 && och_tile_progress_seek(p, 1, 64) != 0, "seek");
    expect(och_tile_progress_feed(p, 1, 32, 8, 0, last.bgra.get(), last.weight.get()) == 0, "a band after seek");
    uint64_t n = 0;
    och_tile_update updates[3];
    std::unique_ptr<uint8_t[]> thumbs(new uint8_t[3 * 32 * 32 * 4]);
    expect(och_tile_progress_collect(p, updates, thumbs.get(), 2, &n) != 0 && n == 3, "a capacity below the band's tiles");
    expect(och_tile_progress_collect(p, updates, nullptr, 3, &n) != 0, "no thumbnails");
    expect(och_tile_progress_pending(p) == 3, "a refused collect keeps the band");
    expect(och_tile_progress_collect(p, updates, thumbs.get(), 3, &n) == 0 && n == 3, "collect");
    och_tile_progress_destroy(p); // with two bands never collected
    och_tile_progress_destroy(nullptr);
}

} // namespace

int main()
{
    std::mt19937 rng(17);
    const int64_t cases[][3] = {{1, 1, 1}, {300, 130, 128}, {260, 129, 129}, {520, 300, 255}, {520, 300, 256}, {520, 300, 257},
                                {1100, 1030, 1024}, {4100, 200, 4096}};
    long rasters = 0;
    for (const auto &c : cases)
        for (int L : {1, 2, 8})
            for (int content = 0; content < 9; content++)
            {
                if (c[0] * c[1] * L > 3000000 && content % 4) // the large shapes: three contents
                    continue;
                run_raster(content, L, c[0], c[1], (int)c[2], content % 2 ? 1 : 2, rng);
                rasters++;
            }
    run_raster(8, 2, 70, 40, 32, 1, rng); // 3 x 2 tiles in two bands
    refusals();
    if (failures)
    {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("tile progress ok: %ld rasters (%s .. %s), the refusals\n", rasters + 1, CONTENTS[0], CONTENTS[8]);
    return 0;
}
