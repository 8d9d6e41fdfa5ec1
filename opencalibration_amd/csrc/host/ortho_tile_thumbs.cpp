// liboc_host.so: per-tile progress of the layer and blend passes (csrc/ortho_tile_thumbs.hpp; the
// reference's TileProgressCallback, src/ortho/ortho.cpp:1553-1614, 1962-2011).  The och_tile_progress_* object: the bands'
// bookkeeping and the TileUpdate records for both routes, the CPU route's loops, and the queue of jobs in flight on the device.
#include "../../../include/oc_host.h"

#include "../ortho_tile_thumbs.hpp"

#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

static_assert(sizeof(och_tile_update) == 72, "och_tile_update is 72 bytes, no padding");

namespace
{
thread_local std::string progress_error;

int fail(int code, const std::string &text)
{
    progress_error = text;
    return code;
}

struct fed_band
{
    int pass = 0;
    int64_t row0 = 0, rows = 0;
    ochip_tile_thumbs_job *job = nullptr; // the device route
    std::vector<uint32_t> slots;          // the CPU route
};
} // namespace

struct och_tile_progress
{
    ochip_ctx *ctx = nullptr;
    int64_t width = 0, height = 0;
    double min_x = 0, max_y = 0, gsd = 0;
    int32_t T = 0, L = 0;
    int64_t next_row[3] = {0, 0, 0}; // per pass: the row its next band starts at
    std::deque<fed_band> queue;
};

namespace
{
int64_t tiles_of(const och_tile_progress *p, const fed_band &b)
{
    return ochip_tt::tiles_along(p->width, p->T) * ochip_tt::tiles_along(b.rows, p->T);
}
} // namespace

extern "C"
{

const char *och_tile_progress_last_error(void)
{
    return progress_error.c_str();
}

int och_tile_progress_create(ochip_ctx *ctx, const double *plan8, int32_t tile_size, int32_t num_layers, och_tile_progress **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_tile_progress_create: out is NULL");
    *out = nullptr;
    if (!plan8)
        return fail(OCHIP_EINVAL, "och_tile_progress_create: the plan is NULL");
    if (!(plan8[0] >= 1 && plan8[0] <= 2147483647.0 && plan8[1] >= 1 && plan8[1] <= 2147483647.0))
        return fail(OCHIP_EINVAL, "och_tile_progress_create: a raster of " + std::to_string(plan8[0]) + " x " + std::to_string(plan8[1]));
    if (tile_size < 1 || tile_size > ochip_tt::MAX_TILE || num_layers < 1 || num_layers > ochip_tt::MAX_LAYERS)
        return fail(OCHIP_EINVAL, "och_tile_progress_create: tile_size " + std::to_string(tile_size) + " (1.." +
                                      std::to_string(ochip_tt::MAX_TILE) + "), num_layers " + std::to_string(num_layers) + " (1.." +
                                      std::to_string(ochip_tt::MAX_LAYERS) + ")");
    std::unique_ptr<och_tile_progress> p(new och_tile_progress);
    p->ctx = ctx;
    p->width = (int64_t)plan8[0], p->height = (int64_t)plan8[1];
    p->gsd = plan8[2], p->min_x = plan8[3], p->max_y = plan8[6];
    p->T = tile_size, p->L = num_layers;
    if (ochip_tt::tiles_along(p->width, p->T) * ochip_tt::tiles_along(p->height, p->T) > 0x7FFFFFFF)
        return fail(OCHIP_EINVAL, "och_tile_progress_create: more than 2^31 - 1 tiles");
    *out = p.release();
    return OCHIP_OK;
}

int och_tile_progress_feed(och_tile_progress *p, int pass, int64_t row0, int64_t rows, int on_device, const uint8_t *pixels,
                           const float *weight)
{
    if (!p)
        return fail(OCHIP_EINVAL, "och_tile_progress_feed: no object");
    const std::string band = "rows " + std::to_string(row0) + " to " + std::to_string(row0 + rows);
    if (pass != ochip_tt::PASS_LAYERS && pass != ochip_tt::PASS_BLEND)
        return fail(OCHIP_EINVAL, "och_tile_progress_feed: pass " + std::to_string(pass) + " is neither 1 (layers) nor 2 (blend)");
    if (rows <= 0 || row0 < 0 || row0 + rows > p->height)
        return fail(OCHIP_EINVAL, "och_tile_progress_feed: " + band + " of a raster of " + std::to_string(p->height) + " rows");
    if (row0 % p->T)
        return fail(OCHIP_EINVAL, "och_tile_progress_feed: " + band + ": row " + std::to_string(row0) + " is not on a tile row (tile_size " +
                                      std::to_string(p->T) + ")");
    if (rows % p->T && row0 + rows != p->height)
        return fail(OCHIP_EINVAL, "och_tile_progress_feed: " + band + " are neither whole tile rows (tile_size " + std::to_string(p->T) +
                                      ") nor the raster's last");
    const int64_t next = p->next_row[pass] == p->height ? 0 : p->next_row[pass]; // a finished sweep: the pass may start again
    if (row0 != next)
        return fail(OCHIP_EINVAL, std::string("och_tile_progress_feed: ") + (row0 > next ? "gap: " : "out of raster order: ") + band +
                                      " of pass " + std::to_string(pass) + " when row " + std::to_string(next) + " is next");
    const std::string why = ochip_tt::refusal(pass, p->width, rows, p->T, p->L, pixels, weight);
    if (!why.empty())
        return fail(OCHIP_EINVAL, "och_tile_progress_feed: " + why);
    fed_band b;
    b.pass = pass, b.row0 = row0, b.rows = rows;
    if (p->ctx)
    {
        const int rc = ochip_ortho_tile_thumbs_enqueue(p->ctx, pass, (int32_t)p->width, rows, p->T, p->L, on_device, pixels, weight, &b.job);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(p->ctx));
    }
    else
    {
        if (on_device)
            return fail(OCHIP_EINVAL, "och_tile_progress_feed: inputs on the device need a device context");
        const ochip_tt::band B{pass, (int32_t)p->width, p->T, p->L, rows, reinterpret_cast<const uint32_t *>(pixels),
                               pass == ochip_tt::PASS_LAYERS ? weight : nullptr};
        b.slots.resize((size_t)B.tiles() * B.slot_pixels());
        ochip_tt::cpu_route(B, b.slots.data());
    }
    p->next_row[pass] = row0 + rows;
    p->queue.push_back(std::move(b));
    return OCHIP_OK;
}

int och_tile_progress_seek(och_tile_progress *p, int pass, int64_t row0)
{
    if (!p)
        return fail(OCHIP_EINVAL, "och_tile_progress_seek: no object");
    if ((pass != ochip_tt::PASS_LAYERS && pass != ochip_tt::PASS_BLEND) || row0 < 0 || row0 >= p->height || row0 % p->T)
        return fail(OCHIP_EINVAL, "och_tile_progress_seek: pass " + std::to_string(pass) + ", row " + std::to_string(row0) +
                                      " is not a tile row (tile_size " + std::to_string(p->T) + ") of a raster of " +
                                      std::to_string(p->height) + " rows");
    p->next_row[pass] = row0;
    return OCHIP_OK;
}

int och_tile_progress_pending(const och_tile_progress *p)
{
    return p ? (int)p->queue.size() : 0;
}

int och_tile_progress_collect(och_tile_progress *p, och_tile_update *updates, uint8_t *thumbs, uint64_t capacity, uint64_t *n)
{
    if (!p || !n)
        return fail(OCHIP_EINVAL, "och_tile_progress_collect: no object or no count");
    *n = 0;
    if (p->queue.empty())
        return fail(OCHIP_EINVAL, "och_tile_progress_collect: no band is pending");
    fed_band &b = p->queue.front();
    const int64_t tiles = tiles_of(p, b);
    *n = (uint64_t)tiles;
    if (!updates)
        return OCHIP_OK;
    if (!thumbs || capacity < (uint64_t)tiles)
        return fail(OCHIP_EINVAL, "och_tile_progress_collect: rows " + std::to_string(b.row0) + " to " + std::to_string(b.row0 + b.rows) +
                                      " of pass " + std::to_string(b.pass) + " are " + std::to_string(tiles) + " tiles, the capacity is " +
                                      std::to_string(thumbs ? capacity : 0));
    const size_t slot_bytes = (size_t)ochip_tt::slot_side(p->T) * (size_t)ochip_tt::slot_side(p->T) * 4;
    if (b.job)
    {
        const uint8_t *src = nullptr;
        uint64_t bytes = 0;
        const int rc = ochip_ortho_tile_thumbs_wait(b.job, &src, &bytes);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(p->ctx));
        std::memcpy(thumbs, src, (size_t)bytes);
        ochip_ortho_tile_thumbs_release(b.job);
        b.job = nullptr;
    }
    else
        std::memcpy(thumbs, b.slots.data(), (size_t)tiles * slot_bytes);
    const int64_t tiles_x = ochip_tt::tiles_along(p->width, p->T), tiles_y = ochip_tt::tiles_along(p->height, p->T);
    const int64_t first_ty = b.row0 / p->T;
    for (int64_t t = 0; t < tiles; t++)
    {
        const int64_t tx = t % tiles_x, ty = t / tiles_x;
        och_tile_update &u = updates[t];
        u.pixel_x = (int32_t)(tx * p->T), u.pixel_y = (int32_t)(b.row0 + ty * p->T);
        u.pixel_w = ochip_tt::tile_extent(p->width, p->T, tx), u.pixel_h = ochip_tt::tile_extent(b.rows, p->T, ty);
        u.total_output_width = (int32_t)p->width, u.total_output_height = (int32_t)p->height;
        u.tile_index = (int32_t)((first_ty + ty) * tiles_x + tx + 1), u.total_tiles = (int32_t)(tiles_x * tiles_y);
        const ochip_tt::thumb_dims d = ochip_tt::dims_of(u.pixel_w, u.pixel_h);
        u.thumb_w = d.w, u.thumb_h = d.h, u.scale = d.scale, u.pass = b.pass;
        u.bounds_min_x = p->min_x, u.bounds_max_y = p->max_y, u.meters_per_pixel = p->gsd;
    }
    p->queue.pop_front();
    return OCHIP_OK;
}

void och_tile_progress_destroy(och_tile_progress *p)
{
    if (!p)
        return;
    for (fed_band &b : p->queue)
        ochip_ortho_tile_thumbs_release(b.job);
    delete p;
}

} // extern "C"
