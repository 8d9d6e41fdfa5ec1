// liboc_host.so: averaged overview levels of the orthomosaic and the DSM (csrc/ortho_overview.hpp; the
// reference's BuildOverviews("AVERAGE", ...) calls, src/ortho/ortho.cpp:944-961, 1642-1657, 2028-2044).  The CPU route - the
// shared header's bookkeeping and cell rules in straight loops, every level one at a time - and the C ABI over both routes.
#include "../../../include/oc_host.h"

#include "../ortho_overview.hpp"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace
{
thread_local std::string overview_error;

int fail(int code, const std::string &text)
{
    overview_error = text;
    return code;
}
} // namespace

struct och_ortho_overviews
{
    ochip_ctx *ctx = nullptr;
    ochip_ortho_overviews *dev = nullptr; // the device route
    // the CPU route
    int kind = 0;
    ochip_ov::progress P;
    std::vector<void *> level; // [1 .. levels], the caller's
    std::vector<uint32_t> pending;
};

namespace
{
template <class R> void run_steps(och_ortho_overviews *o, const std::vector<ochip_ov::step> &steps, int64_t row0, const void *band_host)
{
    using T = typename R::type;
    const ochip_ov::progress &P = o->P;
    const T *band = static_cast<const T *>(band_host);
    for (const ochip_ov::step &s : steps)
    {
        if (s.what == ochip_ov::step::KEEP)
        {
            std::memcpy(o->pending.data(), band + (size_t)(s.r0 - row0) * (size_t)P.width, (size_t)P.width * 4);
            continue;
        }
        const bool first = s.level == 1;
        ochip_ov::level_rows<R>(first ? band : static_cast<const T *>(o->level[s.level - 1]), first ? row0 : 0, P.level_w(s.level - 1),
                                P.level_h(s.level - 1), s.top_pending ? reinterpret_cast<const T *>(o->pending.data()) : nullptr,
                                static_cast<T *>(o->level[s.level]), P.level_w(s.level), s.r0, s.r1);
    }
}
} // namespace

extern "C"
{

const char *och_ortho_overviews_last_error(void)
{
    return overview_error.c_str();
}

int och_ortho_overviews_levels(int64_t width, int64_t height, int64_t *rows_cols)
{
    if (width < 1 || height < 1)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_levels: a raster of " + std::to_string(width) + " x " + std::to_string(height));
    const int n = ochip_ov::num_levels(width, height);
    for (int k = 1; k <= n && rows_cols; k++)
        rows_cols[2 * (k - 1)] = ochip_ov::level_extent(height, k), rows_cols[2 * (k - 1) + 1] = ochip_ov::level_extent(width, k);
    return n;
}

int och_ortho_overviews_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, void *const *levels, int on_device,
                               och_ortho_overviews **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_ortho_overviews> o(new och_ortho_overviews);
    o->ctx = ctx, o->kind = kind;
    if (ctx)
    {
        const int rc = ochip_ortho_overviews_create(ctx, kind, width, height, levels, on_device, &o->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
        *out = o.release();
        return OCHIP_OK;
    }
    if ((kind != ochip_ov::KIND_RGBA8 && kind != ochip_ov::KIND_FLOAT32) || width < 1 || height < 1)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_create: bad argument (" + std::to_string(width) + " x " + std::to_string(height) +
                                      ", kind " + std::to_string(kind) + ")");
    if (on_device)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_create: levels on the device need a device context");
    o->P.reset(width, height);
    o->level.assign((size_t)o->P.levels + 1, nullptr);
    for (int k = 1; k <= o->P.levels; k++)
        if (!levels || !(o->level[k] = levels[k - 1]))
            return fail(OCHIP_EINVAL, "och_ortho_overviews_create: " + std::to_string(width) + " x " + std::to_string(height) + " has " +
                                          std::to_string(o->P.levels) + " levels, the buffer of level " + std::to_string(k) + " is NULL");
    o->pending.resize((size_t)width);
    *out = o.release();
    return OCHIP_OK;
}

int och_ortho_overviews_feed(och_ortho_overviews *o, int64_t row0, int64_t rows, const void *band)
{
    if (!o)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_feed: no builder");
    if (o->dev)
    {
        const int rc = ochip_ortho_overviews_feed(o->dev, row0, rows, band);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(o->ctx));
    }
    if (!band)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_feed: the band is NULL");
    std::vector<ochip_ov::step> steps;
    const std::string refusal = o->P.feed(row0, rows, false, &steps);
    if (!refusal.empty())
        return fail(OCHIP_EINVAL, "och_ortho_overviews_feed: " + refusal);
    if (o->kind == ochip_ov::KIND_RGBA8)
        run_steps<ochip_ov::rgba_rule>(o, steps, row0, band);
    else
        run_steps<ochip_ov::float_rule>(o, steps, row0, band);
    return OCHIP_OK;
}

int64_t och_ortho_overviews_complete_rows(const och_ortho_overviews *o, int level)
{
    if (!o)
        return 0;
    if (o->dev)
        return ochip_ortho_overviews_complete_rows(o->dev, level);
    return level >= 1 && level <= o->P.levels ? o->P.done[level] : 0;
}

int och_ortho_overviews_finish(och_ortho_overviews *o)
{
    if (!o)
        return fail(OCHIP_EINVAL, "och_ortho_overviews_finish: no builder");
    if (o->dev)
    {
        const int rc = ochip_ortho_overviews_finish(o->dev);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(o->ctx));
    }
    const std::string refusal = o->P.finish();
    return refusal.empty() ? OCHIP_OK : fail(OCHIP_EINVAL, "och_ortho_overviews_finish: " + refusal);
}

void och_ortho_overviews_destroy(och_ortho_overviews *o)
{
    if (!o)
        return;
    ochip_ortho_overviews_destroy(o->dev);
    delete o;
}

} // extern "C"
