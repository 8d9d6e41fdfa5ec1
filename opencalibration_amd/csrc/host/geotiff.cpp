// liboc_host.so: the tiles of the tiled DEFLATE GeoTIFFs (csrc/deflate_rules.hpp; the reference's
// createGeoTIFF / createDSMGeoTIFF, src/ortho/ortho.cpp:655-708 and :745-791).  The CPU route - the shared header's rules in
// straight loops, a tile row's tiles under OpenMP - and the C ABI over both routes.  The CPU route never hands a raster to
// the device by size: it is the yardstick of the device route's tests.
#include "../../../include/oc_host.h"

#include "../deflate_rules.hpp"
#include "../live_handles.hpp"

#include <deque>
#include <memory>
#include <string>
#include <vector>

namespace
{
using namespace ochip_df;

thread_local std::string geotiff_error;

int fail(int code, const std::string &text)
{
    geotiff_error = text;
    return code;
}

ochip::live_set<och_geotiff> g_live; // the writers that exist
} // namespace

struct och_geotiff
{
    ochip_ctx *ctx = nullptr;
    ochip_geotiff *dev = nullptr; // the device route
    // the CPU route
    int kind = 0, sparse = 1;
    int layers = 1, unit = 1, px = PIXEL_BYTES; // a pixel: `layers` samples of `unit` 32-bit words, px bytes
    int64_t w = 0, h = 0, tiles_x = 0, next_row = 0;
    bool finished = false;
    std::vector<uint32_t> rows;              // the tile row being filled: [layers][512][w] samples, zeros where nothing was fed
    std::deque<std::vector<uint8_t>> ready; // the streams of the complete tiles, in tile order; empty: a sparse tile
};

namespace
{
// The predicted payload of tile tx of the tile row held in e->rows; returns whether any byte of it is non-zero
bool fill_payload(const och_geotiff *e, int64_t tx, uint8_t *payload)
{
    const bool words = word_predictor(e->kind);
    const int L = e->layers, U = e->unit;
    const size_t row_words = (size_t)e->w * (size_t)U, plane = (size_t)TILE * row_words;
    uint32_t any = 0;
    for (int r = 0; r < TILE; r++)
    {
        uint32_t left[MAX_LAYERS * 2] = {0, 0, 0, 0};
        uint8_t *out = payload + (size_t)r * (size_t)tile_row_bytes(e->px);
        for (int x = 0; x < TILE; x++)
        {
            const int64_t X = tx * TILE + x;
            for (int l = 0; l < L; l++)
                for (int u = 0; u < U; u++, out += 4)
                {
                    const uint32_t cur = X < e->w ? e->rows[(size_t)l * plane + (size_t)r * row_words + (size_t)X * U + u] : 0;
                    const uint32_t v = x == 0 ? cur : predict_word(cur, left[l * U + u], words);
                    std::memcpy(out, &v, 4);
                    any |= cur, left[l * U + u] = cur;
                }
        }
    }
    return any != 0;
}

void encode_tile_row(och_geotiff *e)
{
    std::vector<std::vector<uint8_t>> out((size_t)e->tiles_x);
#pragma omp parallel for schedule(dynamic)
    for (int64_t tx = 0; tx < e->tiles_x; tx++)
    {
        std::vector<uint8_t> payload((size_t)tile_payload(e->px));
        const bool any = fill_payload(e, tx, payload.data());
        if (any || !e->sparse || e->kind == OCH_GEOTIFF_FLOAT32)
            encode_tile(payload.data(), e->px, out[(size_t)tx]);
    }
    for (auto &o : out)
        e->ready.push_back(std::move(o));
    std::fill(e->rows.begin(), e->rows.end(), 0u);
}

std::string refuse_feed(const och_geotiff *e, int64_t row0, int64_t rows)
{
    if (e->finished)
        return "rows " + std::to_string(row0) + " .. " + std::to_string(row0 + rows) + " after finish";
    if (rows < 0 || row0 != e->next_row)
        return "rows " + std::to_string(row0) + " .. " + std::to_string(row0 + rows) + " where row " + std::to_string(e->next_row) +
               " is next (" + (row0 > e->next_row ? "a gap" : "an overlap") + ")";
    if (row0 + rows > e->h)
        return "rows " + std::to_string(row0) + " .. " + std::to_string(row0 + rows) + " beyond the raster's " + std::to_string(e->h);
    return "";
}
} // namespace

extern "C"
{

const char *och_geotiff_last_error(void)
{
    return geotiff_error.c_str();
}

int och_deflate_code_lengths(const uint32_t *counts, int n, int limit, uint8_t *lens)
{
    if (!counts || !lens || n < 0 || n > NUM_LIT || limit < 1 || limit > 15 || (n > 0 && (1 << limit) < n))
        return fail(OCHIP_EINVAL, "och_deflate_code_lengths: up to 286 counts and a limit of 1 .. 15 bits that can hold them");
    block_work W;
    code_lengths(counts, n, limit, lens, W.key, W.sym, W.num);
    return OCHIP_OK;
}

namespace
{
void shape(och_geotiff *e, int kind, int layers, int64_t width, int64_t height, int sparse)
{
    e->kind = kind, e->sparse = sparse != 0, e->w = width, e->h = height, e->tiles_x = (width + TILE - 1) / TILE;
    e->layers = layers, e->unit = unit_words(kind), e->px = pixel_bytes(kind, layers);
    e->rows.assign((size_t)layers * TILE * (size_t)width * (size_t)e->unit, 0u);
}
} // namespace

int och_geotiff_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int sparse, och_geotiff **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_geotiff_create_layered: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_geotiff> e(new och_geotiff);
    e->ctx = ctx;
    if (ctx)
    {
        const int rc = ochip_geotiff_create_layered(ctx, kind, num_layers, width, height, sparse, &e->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
    }
    else
    {
        if (!layered_kind(kind) || num_layers < 1 || num_layers > MAX_LAYERS || width < 1 || height < 1 || width > OCH_GEOTIFF_MAX_SIDE ||
            height > OCH_GEOTIFF_MAX_SIDE)
            return fail(OCHIP_EINVAL, "och_geotiff_create_layered: kind 2 (layers) or 3 (cameras), 1 .. " + std::to_string(MAX_LAYERS) +
                                          " layers and sides of 1 .. " + std::to_string(OCH_GEOTIFF_MAX_SIDE) + ", not kind " +
                                          std::to_string(kind) + ", " + std::to_string(num_layers) + " layers, " + std::to_string(width) +
                                          " x " + std::to_string(height));
        shape(e.get(), kind, num_layers, width, height, sparse);
    }
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

int och_geotiff_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, int sparse, och_geotiff **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_geotiff_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_geotiff> e(new och_geotiff);
    e->ctx = ctx;
    if (ctx)
    {
        const int rc = ochip_geotiff_create(ctx, kind, width, height, sparse, &e->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
    }
    else
    {
        if ((kind != OCH_GEOTIFF_RGBA8 && kind != OCH_GEOTIFF_FLOAT32) || width < 1 || height < 1 || width > OCH_GEOTIFF_MAX_SIDE ||
            height > OCH_GEOTIFF_MAX_SIDE)
            return fail(OCHIP_EINVAL, "och_geotiff_create: kind 0 (RGBA8) or 1 (float32) and sides of 1 .. " +
                                          std::to_string(OCH_GEOTIFF_MAX_SIDE) + ", not kind " + std::to_string(kind) + ", " +
                                          std::to_string(width) + " x " + std::to_string(height));
        shape(e.get(), kind, 1, width, height, sparse);
    }
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

int och_geotiff_feed(och_geotiff *e, int64_t row0, int64_t rows, const void *pixels, int on_device)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_geotiff_feed: not a live och_geotiff object");
    if (e->dev)
    {
        const int rc = ochip_geotiff_feed(e->dev, row0, rows, pixels, on_device);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    if (!pixels)
        return fail(OCHIP_EINVAL, "och_geotiff_feed: the band is NULL");
    if (on_device)
        return fail(OCHIP_EINVAL, "och_geotiff_feed: a band on the device needs a device context");
    const std::string refusal = refuse_feed(e, row0, rows);
    if (!refusal.empty())
        return fail(e->finished ? OCHIP_ESTATE : OCHIP_EINVAL, "och_geotiff_feed: " + refusal);
    const uint8_t *band = static_cast<const uint8_t *>(pixels);
    const size_t row_words = (size_t)e->w * (size_t)e->unit, row_bytes = row_words * 4; // one layer's row
    for (int64_t r = 0; r < rows; r++)
    {
        const int64_t y = row0 + r;
        for (int l = 0; l < e->layers; l++) // the band is layer-major, as the tile row is
            std::memcpy(e->rows.data() + ((size_t)l * TILE + (size_t)(y % TILE)) * row_words,
                        band + ((size_t)l * (size_t)rows + (size_t)r) * row_bytes, row_bytes);
        e->next_row = y + 1;
        if (e->next_row % TILE == 0 || e->next_row == e->h)
            encode_tile_row(e);
    }
    return OCHIP_OK;
}

int och_geotiff_payloads(och_geotiff *e, const uint8_t *payloads, int64_t n)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_geotiff_payloads: not a live och_geotiff object");
    if (e->dev)
    {
        const int rc = ochip_geotiff_payloads(e->dev, payloads, n);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    if (!payloads || n < 0)
        return fail(OCHIP_EINVAL, "och_geotiff_payloads: the payloads are NULL or their number negative");
    std::vector<std::vector<uint8_t>> out((size_t)n);
#pragma omp parallel for schedule(dynamic)
    for (int64_t i = 0; i < n; i++)
        encode_tile(payloads + (size_t)i * (size_t)tile_payload(e->px), e->px, out[(size_t)i]);
    for (auto &o : out)
        e->ready.push_back(std::move(o));
    return OCHIP_OK;
}

int och_geotiff_collect(och_geotiff *e, uint8_t *buf, uint64_t cap, uint64_t *bytes, uint64_t *counts, uint64_t max_tiles,
                        uint64_t *tiles)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_geotiff_collect: not a live och_geotiff object");
    if (!bytes || !tiles)
        return fail(OCHIP_EINVAL, "och_geotiff_collect: no place for the counts");
    if (e->dev)
    {
        const int rc = ochip_geotiff_collect(e->dev, buf, cap, bytes, counts, max_tiles, tiles);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    uint64_t total = 0;
    for (const auto &t : e->ready)
        total += t.size();
    *bytes = total, *tiles = e->ready.size();
    if (!buf && !counts)
        return OCHIP_OK;
    if (!buf || !counts || cap < total || max_tiles < e->ready.size())
        return fail(OCHIP_EINVAL, "och_geotiff_collect: room for " + std::to_string(cap) + " bytes and " + std::to_string(max_tiles) +
                                      " tiles, " + std::to_string(total) + " and " + std::to_string(e->ready.size()) + " are ready");
    size_t at = 0, k = 0;
    for (const auto &t : e->ready)
    {
        if (!t.empty())
            std::memcpy(buf + at, t.data(), t.size());
        counts[k++] = t.size(), at += t.size();
    }
    e->ready.clear();
    return OCHIP_OK;
}

int och_geotiff_finish(och_geotiff *e)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_geotiff_finish: not a live och_geotiff object");
    if (e->dev)
    {
        const int rc = ochip_geotiff_finish(e->dev);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    if (e->finished)
        return fail(OCHIP_ESTATE, "och_geotiff_finish: finished already");
    if (e->next_row != e->h)
        return fail(OCHIP_ESTATE, "och_geotiff_finish: rows " + std::to_string(e->next_row) + " .. " + std::to_string(e->h) + " were never fed");
    e->finished = true;
    return OCHIP_OK;
}

void och_geotiff_destroy(och_geotiff *e)
{
    if (!g_live.remove(e))
        return;
    ochip_geotiff_destroy(e->dev);
    delete e;
}

} // extern "C"
