// A stand-alone run of the JPEG texture's host code (csrc/jpeg_encode.hpp, csrc/host/jpeg_encode.cpp) for the address and
// undefined-behaviour sanitizers.  Every band and every collect buffer is a heap block of exactly its size, so that a read or
// write past either end is caught.  The shapes of the tests (noise, a ramp, flat 255, a checker), the worst case - noise at
// quality 100 -, every raster whole, row by row and in bands of 7 and 17 rows with both pixel strides, each against the
// one-shot bytes; the bounds of jpeg_encode.hpp against what the coder writes; and the refusals.  Host code only; from the
// repository root:
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude scripts/jpeg_encode_sanitize.cpp opencalibration_amd/csrc/host/jpeg_encode.cpp -o jpeg_encode_sanitize
//   ./jpeg_encode_sanitize
//
// The device route is not linked: its entry points that jpeg_encode.cpp names are stubs here and never called.
#include "../include/oc_host.h"
#include "../opencalibration_amd/csrc/jpeg_encode.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

extern "C"
{
int ochip_jpeg_create(ochip_ctx *, int64_t, int64_t, int, ochip_jpeg **)
{
    std::abort();
}
int ochip_jpeg_feed(ochip_jpeg *, int64_t, int64_t, const void *, int, int)
{
    std::abort();
}
int64_t ochip_jpeg_pending(ochip_jpeg *)
{
    std::abort();
}
int ochip_jpeg_collect(ochip_jpeg *, uint8_t *, uint64_t, uint64_t *)
{
    std::abort();
}
int ochip_jpeg_finish(ochip_jpeg *)
{
    std::abort();
}
void ochip_jpeg_destroy(ochip_jpeg *e)
{
    if (e)
        std::abort();
}
const char *ochip_last_error(const ochip_ctx *)
{
    return "";
}
}

static int failures = 0;

#define EXPECT(cond)                                                                                                   \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(cond))                                                                                                   \
        {                                                                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            failures++;                                                                                                \
        }                                                                                                              \
    } while (0)

static std::vector<uint8_t> raster(int kind, int h, int w, int stride, unsigned seed)
{
    std::vector<uint8_t> px((size_t)h * w * stride);
    std::mt19937 rng(seed);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
        {
            uint8_t *p = px.data() + ((size_t)y * w + x) * stride;
            for (int c = 0; c < 3; c++)
                p[c] = kind == 0   ? (uint8_t)(rng() & 255)
                       : kind == 1 ? (uint8_t)(((c == 0 ? 5 * x + 3 * y : c == 1 ? 2 * x + 7 * y : x + y)) % 256)
                       : kind == 2 ? 255
                                   : ((x + y) % 2 ? 156 : 100);
            if (stride == 4)
                p[3] = (uint8_t)(rng() & 255);
        }
    return px;
}

static void take(och_jpeg *e, std::vector<uint8_t> &file)
{
    uint64_t n = 0;
    EXPECT(och_jpeg_collect(e, nullptr, 0, &n) == OCHIP_OK);
    EXPECT((int64_t)n == och_jpeg_pending(e));
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]); // exactly the bytes that are ready
    uint64_t got = 0;
    EXPECT(och_jpeg_collect(e, buf.get(), n, &got) == OCHIP_OK && got == n);
    file.insert(file.end(), buf.get(), buf.get() + n);
}

// the file of a raster fed in bands of `step` rows, every band copied into a block of exactly its size
static std::vector<uint8_t> encode(const std::vector<uint8_t> &px, int h, int w, int stride, int quality, int step, bool collect_each)
{
    std::vector<uint8_t> file;
    och_jpeg *e = nullptr;
    EXPECT(och_jpeg_create(nullptr, w, h, quality, &e) == OCHIP_OK);
    if (!e)
        return file;
    for (int r = 0; r < h; r += step)
    {
        const int rows = r + step <= h ? step : h - r;
        const size_t bytes = (size_t)rows * w * stride;
        std::unique_ptr<uint8_t[]> band(new uint8_t[bytes]);
        std::memcpy(band.get(), px.data() + (size_t)r * w * stride, bytes);
        EXPECT(och_jpeg_feed(e, r, rows, band.get(), stride, 0) == OCHIP_OK);
        if (collect_each)
            take(e, file);
    }
    EXPECT(och_jpeg_finish(e) == OCHIP_OK);
    take(e, file);
    och_jpeg_destroy(e);
    return file;
}

static void check_shapes()
{
    const int shapes[][2] = {{1, 1}, {2, 2}, {8, 8}, {16, 16}, {8, 16}, {16, 8}, {7, 25}, {25, 7}, {9, 17}, {17, 9}, {15, 15}, {24, 40},
                             {40, 24}, {31, 33}, {33, 47}, {48, 64}, {64, 80}, {131, 23}};
    for (const auto &s : shapes)
        for (int kind = 0; kind < 4; kind++)
        {
            const int h = s[0], w = s[1], quality = kind == 3 ? 50 : 95;
            const std::vector<uint8_t> rgb = raster(kind, h, w, 3, (unsigned)(h * 131 + w));
            std::vector<uint8_t> rgba((size_t)h * w * 4, 77);
            for (size_t i = 0; i < (size_t)h * w; i++)
                std::memcpy(rgba.data() + 4 * i, rgb.data() + 3 * i, 3);
            const std::vector<uint8_t> whole = encode(rgb, h, w, 3, quality, h, false);
            EXPECT(whole.size() > 600 && whole[0] == 0xFF && whole[1] == 0xD8 && whole[whole.size() - 2] == 0xFF && whole.back() == 0xD9);
            for (int step : {1, 7, 17})
            {
                EXPECT(encode(rgb, h, w, 3, quality, step, true) == whole);
                EXPECT(encode(rgba, h, w, 4, quality, step, step == 7) == whole);
            }
        }
}

// noise at quality 100 stays inside the bound the buffers are sized from, and the bound is not far from what occurs
static void check_worst_case()
{
    const int h = 64, w = 96;
    const std::vector<uint8_t> px = raster(0, h, w, 3, 9);
    const std::vector<uint8_t> file = encode(px, h, w, 3, 100, 1, true);
    const size_t mcus = (size_t)(h / 16) * (w / 16), header = 623;
    EXPECT(file.size() > header + mcus * 300);
    EXPECT(file.size() <= header + 2 * (mcus * ochip_jp::MCU_MAX_BYTES + 1) + 2);
    // every symbol of one block at its longest: 16-bit codes with 11 / 10 bits behind them
    ochip_jp::tables t;
    ochip_jp::build_tables(100, t);
    ochip_jp::bit_counter bits;
    ochip_jp::block_coder<ochip_jp::bit_counter> coder(bits, t.dc[0], t.ac[0]);
    coder.dc(-2047);
    for (int k = 1; k < 64; k++)
        coder.ac(k % 2 ? 1023 : -1023);
    coder.end();
    EXPECT(bits.bits == (uint32_t)ochip_jp::BLOCK_MAX_BITS);
}

static void check_refusals()
{
    och_jpeg *e = nullptr;
    EXPECT(och_jpeg_create(nullptr, 0, 4, 95, &e) == OCHIP_EINVAL && !e);
    EXPECT(och_jpeg_create(nullptr, 4, 0, 95, &e) == OCHIP_EINVAL && !e);
    EXPECT(och_jpeg_create(nullptr, 65501, 4, 95, &e) == OCHIP_EINVAL && !e);
    EXPECT(och_jpeg_create(nullptr, 4, 65501, 95, &e) == OCHIP_EINVAL && !e);
    EXPECT(och_jpeg_create(nullptr, 4, 4, 0, &e) == OCHIP_EINVAL && !e);
    EXPECT(och_jpeg_create(nullptr, 4, 4, 101, &e) == OCHIP_EINVAL && !e);
    EXPECT(och_jpeg_create(nullptr, 4, 4, 95, nullptr) == OCHIP_EINVAL);
    EXPECT(std::strstr(och_jpeg_last_error(), "out is NULL") != nullptr);
    const int h = 40, w = 24;
    const std::vector<uint8_t> px = raster(1, h, w, 3, 0);
    EXPECT(och_jpeg_create(nullptr, w, h, 95, &e) == OCHIP_OK && e);
    auto rows = [&](int r0, int n) {
        std::unique_ptr<uint8_t[]> band(new uint8_t[(size_t)n * w * 3]);
        std::memcpy(band.get(), px.data() + (size_t)(r0 % h) * w * 3, (size_t)(r0 % h + n <= h ? n : h - r0 % h) * w * 3);
        return och_jpeg_feed(e, r0, n, band.get(), 3, 0);
    };
    EXPECT(rows(8, 8) == OCHIP_EINVAL && std::strstr(och_jpeg_last_error(), "gap"));
    EXPECT(och_jpeg_feed(e, 0, 20, nullptr, 3, 0) == OCHIP_EINVAL);
    EXPECT(och_jpeg_feed(e, 0, 20, px.data(), 5, 0) == OCHIP_EINVAL);
    EXPECT(och_jpeg_feed(e, 0, 20, px.data(), 3, 1) == OCHIP_EINVAL);
    EXPECT(rows(0, 0) == OCHIP_EINVAL);
    EXPECT(rows(0, 20) == OCHIP_OK);
    EXPECT(rows(16, 8) == OCHIP_EINVAL && std::strstr(och_jpeg_last_error(), "overlap"));
    EXPECT(rows(20, 21) == OCHIP_EINVAL);
    EXPECT(och_jpeg_finish(e) == OCHIP_ESTATE);
    uint64_t n = 0;
    uint8_t small[5];
    EXPECT(och_jpeg_collect(e, small, 5, &n) == OCHIP_EINVAL && n > 600);
    EXPECT(och_jpeg_collect(e, small, 5, nullptr) == OCHIP_EINVAL);
    EXPECT(rows(20, 20) == OCHIP_OK);
    EXPECT(och_jpeg_finish(e) == OCHIP_OK);
    EXPECT(och_jpeg_finish(e) == OCHIP_ESTATE);
    EXPECT(rows(40, 1) == OCHIP_ESTATE);
    std::vector<uint8_t> file;
    take(e, file);
    EXPECT(file == encode(px, h, w, 3, 95, h, false)); // the refusals changed nothing
    och_jpeg_destroy(e);
    EXPECT(och_jpeg_feed(e, 0, 1, px.data(), 3, 0) == OCHIP_EINVAL); // a dead handle is refused, not followed
    EXPECT(och_jpeg_finish(e) == OCHIP_EINVAL && och_jpeg_pending(e) == 0);
    EXPECT(och_jpeg_collect(e, nullptr, 0, &n) == OCHIP_EINVAL);
    och_jpeg_destroy(e);
    och_jpeg_destroy(nullptr);
}

int main()
{
    check_shapes();
    check_worst_case();
    check_refusals();
    std::printf(failures ? "%d checks failed\n" : "jpeg_encode_sanitize: all checks passed\n", failures);
    return failures ? 1 : 0;
}
