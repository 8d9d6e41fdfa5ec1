// liboc_host.so: C ABI of the orthomosaic preview and the DSM raster (ortho.hpp).
#include "../../../include/oc_host.h"

#include "capi_graph.hpp"
#include "ortho.hpp"

#include <cmath>
#include <cstring>

using namespace opencalibration_amd;

namespace
{

thread_local std::string ortho_error;

std::vector<const surface_model *> surface_list(const och_surface *const *surfaces, size_t n)
{
    std::vector<const surface_model *> out;
    for (size_t i = 0; i < n; i++)
        out.push_back(&surfaces[i]->s);
    return out;
}

void write_plan(const ortho::Plan &p, double *plan8)
{
    const double v[8] = {(double)p.width, (double)p.height, p.gsd, p.bounds.min_x, p.bounds.max_x, p.bounds.min_y, p.bounds.max_y,
                         p.mean_camera_z};
    std::memcpy(plan8, v, sizeof v);
}

bool read_plan(const double *plan8, ortho::Plan *p)
{
    if (!(plan8[0] >= 0 && plan8[0] <= 2147483647.0 && plan8[1] >= 0 && plan8[1] <= 2147483647.0))
        return false;
    p->width = (int)plan8[0];
    p->height = (int)plan8[1];
    p->gsd = plan8[2];
    p->bounds = ortho::Bounds{plan8[3], plan8[4], plan8[5], plan8[6], 0};
    p->mean_camera_z = plan8[7];
    return true;
}

int upload_mesh(ochip_ctx *ctx, const std::vector<const surface_model *> &surfaces, ochip_ortho_mesh **out)
{
    const ortho::TriangleTable t = ortho::triangleTable(surfaces);
    const int rc = ochip_ortho_mesh_create(ctx, (uint32_t)surfaces.size(), t.tri_off.data(), t.tri9.empty() ? nullptr : t.tri9.data(),
                                           out);
    if (rc != OCHIP_OK)
        ortho_error = ochip_last_error(ctx);
    return rc;
}

} // namespace

extern "C"
{

int och_graph_set_thumbnail(och_graph *g, size_t node_index, size_t rows, size_t cols, const uint8_t *rgb)
{
    // the device samples thumbnails of at most 65535 x 65535 (ochip_ortho_thumbnail): refused here, before any product
    // of the two can overflow
    if (node_index >= g->graph.size_nodes() || rows > 65535 || cols > 65535 || (rows == 0) != (cols == 0) ||
        (rows != 0 && !rgb))
    {
        g->error = "och_graph_set_thumbnail: bad node index, or a thumbnail size outside 1..65535 x 1..65535 (0 x 0 clears)";
        return -1;
    }
    image &p = g->graph.nodes()[node_index].payload;
    p.thumbnail_rows = rows;
    p.thumbnail_cols = cols;
    p.thumbnail_pixels.assign(rgb, rgb + rows * cols * 3);
    return 0;
}

void och_ortho_bounds(const och_surface *const *surfaces, size_t n, double *bounds5)
{
    const ortho::Bounds b = ortho::calculateBoundsAndMeanZ(surface_list(surfaces, n));
    const double v[5] = {b.min_x, b.max_x, b.min_y, b.max_y, b.mean_surface_z};
    std::memcpy(bounds5, v, sizeof v);
}

double och_ortho_gsd(const och_graph *g, const uint64_t *node_ids, size_t n_ids, double mean_surface_z, int thumbnail)
{
    std::vector<size_t> idx;
    for (size_t i = 0; i < n_ids; i++)
        if (g->graph.getNode(node_ids[i]))
            idx.push_back(g->graph.nodeIndex(node_ids[i]));
    return ortho::calculateGSD(g->graph, idx, mean_surface_z, thumbnail != 0);
}

size_t och_ortho_context(const och_graph *g, const och_surface *const *surfaces, size_t n, int thumbnail, double *ctx8)
{
    const ortho::Context c = ortho::prepareContext(surface_list(surfaces, n), g->graph, thumbnail != 0);
    const double v[8] = {c.bounds.min_x, c.bounds.max_x, c.bounds.min_y, c.bounds.max_y, c.bounds.mean_surface_z,
                         c.gsd, c.mean_camera_z, c.average_camera_elevation};
    std::memcpy(ctx8, v, sizeof v);
    return c.involved.size();
}

void och_ortho_clamp_resolution(uint64_t total_input_pixels, double *gsd, int32_t *width, int32_t *height)
{
    int w = *width, h = *height;
    ortho::clampOutputResolution(*gsd, w, h, total_input_pixels);
    *width = w, *height = h;
}

void och_ortho_clamp_megapixels(double max_output_megapixels, double *gsd, int32_t *width, int32_t *height)
{
    int w = *width, h = *height;
    ortho::clampOutputMegapixels(*gsd, w, h, max_output_megapixels);
    *width = w, *height = h;
}

double och_ray_trace_height(const och_surface *const *surfaces, size_t n, double x, double y, double mean_camera_z)
{
    return ortho::rayTraceHeight(x, y, mean_camera_z, surface_list(surfaces, n));
}

int och_orthomosaic_thumbnail(och_graph *g, ochip_ctx *ctx, const och_surface *const *surfaces, size_t n, const double *z_in,
                              double *plan8, uint8_t *rgba, uint32_t *ids, double *z_out)
{
    const auto surf = surface_list(surfaces, n);
    const ortho::Context context = ortho::prepareContext(surf, g->graph, true);
    const ortho::Plan plan = ortho::thumbnailPlan(context, g->graph);
    write_plan(plan, plan8);
    if (!rgba) // size query
        return 0;
    if (!ids)
    {
        g->error = "och_orthomosaic_thumbnail: ids is NULL";
        return -1;
    }
    ortho::Cameras cams;
    if (!ortho::cameras(context, g->graph, &cams, &g->error))
        return -1;
    const size_t px = (size_t)plan.width * plan.height;
    if (ctx)
    {
        ochip_ortho_mesh *mesh = nullptr;
        if (upload_mesh(ctx, surf, &mesh) != OCHIP_OK)
        {
            g->error = ortho_error;
            return -1;
        }
        const double raster4[4] = {plan.bounds.min_x, plan.bounds.max_y, plan.gsd, plan.mean_camera_z};
        const int rc = ochip_ortho_thumbnail(mesh, raster4, plan.width, plan.height, (uint32_t)cams.ids.size(), cams.cams24.data(),
                                             cams.ids.data(), cams.thumb_off.data(), cams.thumbs.data(), cams.thumbs.size(), rgba, ids,
                                             z_out, nullptr);
        if (rc != OCHIP_OK)
            g->error = ochip_last_error(ctx);
        ochip_ortho_mesh_destroy(mesh);
        return rc == OCHIP_OK ? 0 : -1;
    }
    std::vector<double> z;
    if (z_in)
        z.assign(z_in, z_in + px);
    else
    {
        z.resize(px);
        ortho::heightsCPU(surf, plan, 0, plan.height, z.data(), nullptr, nullptr);
    }
    ortho::colourCPU(plan, cams, z.data(), rgba, ids);
    if (z_out)
        std::copy(z.begin(), z.end(), z_out);
    return 0;
}

int och_dsm_plan(const och_graph *g, const och_surface *const *surfaces, size_t n, double max_output_megapixels, double *plan8)
{
    const ortho::Context context = ortho::prepareContext(surface_list(surfaces, n), g->graph, false);
    write_plan(ortho::dsmPlan(context, g->graph, max_output_megapixels), plan8);
    return 0;
}

int och_ortho_mesh_upload(ochip_ctx *ctx, const och_surface *const *surfaces, size_t n, ochip_ortho_mesh **out)
{
    if (!ctx || !out)
    {
        ortho_error = "och_ortho_mesh_upload: bad argument";
        return -1;
    }
    return upload_mesh(ctx, surface_list(surfaces, n), out) == OCHIP_OK ? 0 : -1;
}

int och_dsm_render(ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces, size_t n, const double *plan8, int64_t row0,
                   int64_t rows, float *out, int out_on_device, uint32_t *tri_out, double *z64_out, uint64_t *capped_walks)
{
    ortho::Plan plan;
    if (!read_plan(plan8, &plan) || row0 < 0 || rows < 0 || row0 + rows > plan.height || (rows && plan.width && !out))
    {
        ortho_error = "och_dsm_render: bad plan, rows or output";
        return -1;
    }
    if (capped_walks)
        *capped_walks = 0;
    if (dev)
    {
        if (!ctx)
        {
            ortho_error = "och_dsm_render: the device route needs the mesh's context";
            return -1;
        }
        const double raster4[4] = {plan.bounds.min_x, plan.bounds.max_y, plan.gsd, plan.mean_camera_z};
        const int rc = ochip_ortho_dsm(dev, raster4, plan.width, row0, rows, out, out_on_device, tri_out, z64_out);
        if (rc != OCHIP_OK)
        {
            ortho_error = std::string("ochip_ortho_dsm: ") + ochip_last_error(ctx);
            return -1;
        }
        return 0;
    }
    if (out_on_device)
    {
        ortho_error = "och_dsm_render: the CPU route writes host memory only";
        return -1;
    }
    const auto surf = surface_list(surfaces, n);
    const ortho::TriangleTable table = tri_out ? ortho::triangleTable(surf) : ortho::TriangleTable{};
    std::vector<double> z((size_t)rows * plan.width);
    const uint64_t capped = ortho::heightsCPU(surf, plan, row0, rows, z.data(), tri_out, tri_out ? &table : nullptr);
    for (size_t i = 0; i < z.size(); i++)
        out[i] = (float)z[i];
    if (z64_out)
        std::copy(z.begin(), z.end(), z64_out);
    if (capped_walks)
        *capped_walks = capped;
    return 0;
}

const char *och_ortho_last_error(void)
{
    return ortho_error.c_str();
}

} // extern "C"
