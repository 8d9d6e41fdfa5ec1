// liboc_host.so: reading the tiles of tiled DEFLATE GeoTIFFs (csrc/inflate_rules.hpp; the reference
// opens orthomosaic.tif and dsm.tif through GDAL, src/ortho/ortho.cpp:2052-2123 and :1735-1756).  The host route - the shared
// header's rules in straight loops, a tile or a stream a thread under OpenMP: inflate, un-predict, place - and the C ABI over
// both routes.  The host route never hands a request to the device by size: it is the yardstick of the device route's
// tests.  With OCHIP_GEOTIFF_READ_STANDALONE defined the device route is left out and the file builds without libochip.so,
// for a stand-alone program under the sanitizers.
#include "../../../include/oc_host.h"

#include "../inflate_rules.hpp"
#include "../live_handles.hpp"

#include <memory>
#include <string>
#include <vector>

namespace
{
using namespace ochip_inf;

thread_local std::string read_error;

int fail(int code, const std::string &text)
{
    read_error = text;
    return code;
}

ochip::live_set<och_geotiff_reader> g_live; // the readers that exist
} // namespace

struct och_geotiff_reader
{
    ochip_ctx *ctx = nullptr;
    ochip_geotiff_reader *dev = nullptr; // the device route
    tile_layout L;                       // the host route
};

extern "C"
{

const char *och_geotiff_read_last_error(void)
{
    return read_error.c_str();
}

int och_geotiff_reader_create(ochip_ctx *ctx, int samples, int is_float, int64_t width, int64_t height, int tile_w, int tile_h, int predictor,
                              uint64_t scratch_budget, och_geotiff_reader **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_geotiff_reader_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_geotiff_reader> r(new och_geotiff_reader);
    r->ctx = ctx;
    if (ctx)
    {
#ifdef OCHIP_GEOTIFF_READ_STANDALONE
        return fail(OCHIP_EINVAL, "och_geotiff_reader_create: built without the device route");
#else
        const int rc = ochip_geotiff_reader_create(ctx, samples, is_float, width, height, tile_w, tile_h, predictor, scratch_budget, &r->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
#endif
    }
    else
    {
        tile_layout &L = r->L;
        L.samples = samples, L.is_float = is_float != 0, L.tile_w = tile_w, L.tile_h = tile_h, L.predictor = predictor;
        L.width = width, L.height = height;
        if (const char *why = refuse_layout(L))
            return fail(OCHIP_EINVAL, std::string("och_geotiff_reader_create: ") + why);
    }
    g_live.add(r.get());
    *out = r.release();
    return OCHIP_OK;
}

int och_geotiff_reader_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int tile_w, int tile_h,
                                      int predictor, uint64_t scratch_budget, och_geotiff_reader **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_geotiff_reader_create_layered: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_geotiff_reader> r(new och_geotiff_reader);
    r->ctx = ctx;
    if (ctx)
    {
#ifdef OCHIP_GEOTIFF_READ_STANDALONE
        return fail(OCHIP_EINVAL, "och_geotiff_reader_create_layered: built without the device route");
#else
        const int rc = ochip_geotiff_reader_create_layered(ctx, kind, num_layers, width, height, tile_w, tile_h, predictor, scratch_budget, &r->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
#endif
    }
    else
    {
        tile_layout &L = r->L;
        if (const char *why = layered_layout(L, kind, num_layers, width, height, tile_w, tile_h, predictor))
            return fail(OCHIP_EINVAL, std::string("och_geotiff_reader_create_layered: ") + why);
    }
    g_live.add(r.get());
    *out = r.release();
    return OCHIP_OK;
}

int och_geotiff_reader_inflate(och_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets, const uint64_t *expect,
                               uint8_t *out, uint64_t out_cap, int32_t *status, uint64_t *bytes)
{
    if (!g_live.has(r))
        return fail(OCHIP_EINVAL, "och_geotiff_reader_inflate: not a live och_geotiff_reader object");
#ifndef OCHIP_GEOTIFF_READ_STANDALONE
    if (r->dev)
    {
        const int rc = ochip_geotiff_reader_inflate(r->dev, n, streams, offsets, expect, out, out_cap, status, bytes);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(r->ctx));
    }
#endif
    if (const char *why = refuse_inflate(n, streams, offsets, expect, out, out_cap, status, bytes))
        return fail(OCHIP_EINVAL, std::string("och_geotiff_reader_inflate: ") + why);
    std::vector<uint64_t> at((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; i++)
        at[(size_t)i + 1] = at[(size_t)i] + slot_of(expect[i]);
#pragma omp parallel for schedule(dynamic)
    for (int64_t i = 0; i < n; i++)
    {
        const stream_result R = inflate_stream(streams + offsets[i], offsets[i + 1] - offsets[i], out + at[(size_t)i], expect[i]);
        status[i] = R.status, bytes[i] = R.bytes;
    }
    return OCHIP_OK;
}

int och_geotiff_reader_read(och_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets, int64_t row0, int64_t rows,
                            void *raster, int on_device, int64_t *bad_tile)
{
    if (!g_live.has(r))
        return fail(OCHIP_EINVAL, "och_geotiff_reader_read: not a live och_geotiff_reader object");
#ifndef OCHIP_GEOTIFF_READ_STANDALONE
    if (r->dev)
    {
        const int rc = ochip_geotiff_reader_read(r->dev, n, streams, offsets, row0, rows, raster, on_device, bad_tile);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(r->ctx));
    }
#endif
    const tile_layout &L = r->L;
    if (const char *why = refuse_read(L, n, streams, offsets, row0, rows, raster, bad_tile))
        return fail(OCHIP_EINVAL, std::string("och_geotiff_reader_read: ") + why);
    if (on_device)
        return fail(OCHIP_EINVAL, "och_geotiff_reader_read: a raster on the device needs a device context");
    *bad_tile = -1;
    const int64_t tiles_x = L.tiles_x(), ty0 = row0 / L.tile_h;
    int64_t bad = n;
#pragma omp parallel
    {
        std::vector<uint8_t> payload((size_t)L.tile_bytes());
#pragma omp for schedule(dynamic) reduction(min : bad)
        for (int64_t i = 0; i < n; i++)
        {
            const uint64_t size = offsets[i + 1] - offsets[i];
            if (size && inflate_stream(streams + offsets[i], size, payload.data(), L.tile_bytes()).status != INF_OK)
            {
                bad = bad < i ? bad : i;
                continue;
            }
            place_tile(L, size ? payload.data() : nullptr, i % tiles_x, ty0 + i / tiles_x, row0, rows, static_cast<uint8_t *>(raster));
        }
    }
    if (bad < n)
        *bad_tile = bad;
    return OCHIP_OK;
}

int64_t och_geotiff_reader_launches(och_geotiff_reader *r)
{
    if (!g_live.has(r))
        return -1;
#ifndef OCHIP_GEOTIFF_READ_STANDALONE
    if (r->dev)
        return ochip_geotiff_reader_launches(r->dev);
#endif
    return 0;
}

void och_geotiff_reader_destroy(och_geotiff_reader *r)
{
    if (!g_live.remove(r))
        return;
#ifndef OCHIP_GEOTIFF_READ_STANDALONE
    ochip_geotiff_reader_destroy(r->dev);
#endif
    delete r;
}

} // extern "C"
