// The surfaces' triangle table on the device (ochip_ortho_mesh, built by ochip_ortho_mesh_create in ortho.hip) and the
// height lookup over it, shared by the preview / DSM kernels (ortho.hip) and the layered render (ortho_layers.hip).
#pragma once

#include "ctx.hpp"
#include "ortho_geom.hpp"

#include <cmath>

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

// the rasters' tiling, shared by the preview / DSM kernels and the layered render
constexpr int TILE = 16; // pixels per tile side; one workgroup of 256 threads per tile

struct raster_args
{
    double min_x, max_y, gsd, mean_camera_z;
    int64_t row0, rows; // rows of this launch (band), from row0 of the raster
    int32_t cols;
    uint32_t tiles_x;
};

inline raster_args make_raster(const double *raster4, int32_t cols, int64_t row0, int64_t rows)
{
    raster_args R;
    R.min_x = raster4[0], R.max_y = raster4[1], R.gsd = raster4[2], R.mean_camera_z = raster4[3];
    R.row0 = row0, R.rows = rows, R.cols = cols;
    R.tiles_x = (uint32_t)((cols + TILE - 1) / TILE);
    return R;
}

// enqueue the device-to-host copy of an output on the context's stream (dst == nullptr: the caller did not ask for it)
inline int copy_back(ochip_ctx *ctx, void *dst, const void *src, size_t bytes, const char *what)
{
    if (dst && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "hipMemcpyAsync failed (%s)", what);
    return OCHIP_OK;
}

} // namespace ochip_om

struct ochip_ortho_mesh
{
    ochip_ctx *ctx = nullptr;
    uint32_t n_surfaces = 0, n_tris = 0;
    ochip_om::ortho_surf *surf = nullptr;
    uint32_t *cell_start = nullptr, *cell_tris = nullptr;
    double *tris = nullptr;
    ochip::dev_blocks mem;
    ochip_om::mesh_args args() const
    {
        return ochip_om::mesh_args{surf, cell_start, cell_tris, tris, n_surfaces};
    }
};

