// The surfaces' triangle table on the device (ochip_ortho_mesh, built by ochip_ortho_mesh_create in ortho.hip) and the
// height lookup over it, shared by the preview / DSM kernels (ortho.hip) and the layered render (ortho_layers.hip).
#pragma once

#include "ctx.hpp"
#include "ortho_geom.hpp"

#include <cmath>
#include <utility>
#include <vector>

namespace ochip_om
{

constexpr uint32_t MISS = 0xFFFFFFFFu;

struct ortho_surf
{
    double ox, oy, cell;
    int32_t ncx, ncy;
    uint32_t cell_base; // this surface's ncx * ncy + 1 cell starts begin at cell_start[cell_base]
};

struct mesh_args
{
    const ortho_surf *surf;
    const uint32_t *cell_start, *cell_tris;
    const double *tris; // [n_tris][9]
    uint32_t n_surfaces;
};

// first surface, then first triangle of the pixel's cell (ascending index) that holds (x, y)
__device__ __forceinline__ uint32_t mesh_height(const mesh_args &M, double x, double y, double mean_camera_z, double *z)
{
    for (uint32_t s = 0; s < M.n_surfaces; s++)
    {
        const ortho_surf S = M.surf[s];
        const int cx = ochip_og::grid_cell(x, S.ox, S.cell, S.ncx), cy = ochip_og::grid_cell(y, S.oy, S.cell, S.ncy);
        if (cx < 0 || cy < 0)
            continue;
        const uint32_t c = S.cell_base + (uint32_t)cy * (uint32_t)S.ncx + (uint32_t)cx;
        const uint32_t end = M.cell_start[c + 1];
        for (uint32_t k = M.cell_start[c]; k < end; k++)
        {
            const uint32_t t = M.cell_tris[k];
            if (ochip_og::triangle_height(M.tris + 9 * (size_t)t, x, y, mean_camera_z, z))
                return t;
        }
    }
    *z = NAN;
    return MISS;
}

inline int pool_upload(ochip_ctx *ctx, std::vector<std::pair<void *, size_t>> &blocks, void **dst, const void *src, size_t bytes)
{
    size_t got = 0;
    void *d = ochip_pool_get(ctx, bytes ? bytes : 16, &got);
    if (!d)
        return ochip_fail(ctx, OCHIP_ENOMEM, "device allocation of %zu bytes failed (ortho)", bytes);
    blocks.emplace_back(d, got);
    if (src && bytes && hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "hipMemcpyAsync failed (ortho)");
    *dst = d;
    return OCHIP_OK;
}

inline void pool_release(ochip_ctx *ctx, std::vector<std::pair<void *, size_t>> &blocks)
{
    for (auto &b : blocks)
        ochip_pool_put(ctx, b.first, b.second);
    blocks.clear();
}

} // namespace ochip_om

struct ochip_ortho_mesh
{
    ochip_ctx *ctx = nullptr;
    uint32_t n_surfaces = 0, n_tris = 0;
    ochip_om::ortho_surf *surf = nullptr;
    uint32_t *cell_start = nullptr, *cell_tris = nullptr;
    double *tris = nullptr;
    std::vector<std::pair<void *, size_t>> blocks;
    ochip_om::mesh_args args() const
    {
        return ochip_om::mesh_args{surf, cell_start, cell_tris, tris, n_surfaces};
    }
};

