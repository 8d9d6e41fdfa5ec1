// libochip.so — the preview orthomosaic and the DSM raster (reference: generateOrthomosaic, src/ortho/ortho.cpp:
// 478-653, and computeDSMTile, :793-856): per output pixel the height of the mesh under the pixel centre
// (x = col * gsd + min_x, y = max_y - row * gsd), the first surface that holds it winning; for the preview also the colour
// of the first of the 5 nearest cameras that sees the point inside its thumbnail.
//
// The reference finds the triangle with a MeshIntersectionSearcher walking from the previous pixel's triangle.  Here the
// host hands over the surfaces' triangles (corners in ascending node order, ortho_geom.hpp) and ochip_ortho_mesh_create
// bins them into one uniform grid per surface (a triangle goes to every cell its bounding box touches, ascending triangle
// order within a cell); a pixel tests the triangles of its cell in that order and takes the first that contains it.
// Pixels are handed out in 16 x 16 tiles per workgroup (16 x 4 per wavefront), so a wavefront's lanes mostly read one
// cell's list.  Everything is fp64 with the walker's predicates and plane arithmetic (ortho_geom.hpp).
#include "ctx.hpp"
#include "ortho_geom.hpp"
#include "ortho_mesh.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace ochip_om;

namespace
{

constexpr int KNN = ochip_og::KNN; // context.imageGPSLocations.searchKnn({x, y}, 5) (ortho.cpp:586)
constexpr int CAM_DOUBLES = 24;          // ochip_ortho_thumbnail's camera record
constexpr uint32_t CAM_LDS_CHUNK = 1024; // camera XY staged in LDS per trip (16 KiB)

__device__ __forceinline__ bool tile_pixel(const raster_args &R, int *col, int64_t *row)
{
    const uint32_t b = blockIdx.x;
    const uint32_t tx = b % R.tiles_x, ty = b / R.tiles_x;
    *col = (int)(tx * TILE + (threadIdx.x & (TILE - 1)));
    const int64_t lr = (int64_t)ty * TILE + (threadIdx.x / TILE);
    *row = R.row0 + lr;
    return *col < R.cols && lr < R.rows;
}

// image_from_3d(ray, model) (include/opencalibration/distort/distort_keypoints.hpp:45-67) with the PLANAR projection: z
// clamped to 1e-3, radial and tangential distortion (distortProjectedRay, :26-42), * f + principal point.  cam + 12:
// f, ppx, ppy, k1, k2, k3, p1, p2.
__device__ __forceinline__ void camera_project(const double *cam, const double ray[3], double pixel[2])
{
    const double *m = cam + 12; // f ppx ppy k1 k2 k3 p1 p2
    const double z = ray[2] < 1e-3 ? 1e-3 : ray[2];
    const double p[2] = {ray[0] / z, ray[1] / z};
    double r2[3];
    r2[0] = p[0] * p[0] + p[1] * p[1];
    r2[1] = r2[0] * r2[0];
    r2[2] = r2[1] * r2[0];
    const double *k = m + 3, *t = m + 6;
    const double radial = k[0] * r2[0] + k[1] * r2[1] + k[2] * r2[2];
    const double prod = p[0] * p[1];
    for (int i = 0; i < 2; i++)
    {
        const double dd = (1.0 + radial) * p[i] + 2.0 * prod * t[i] + t[1 - i] * (r2[0] + 2.0 * p[i] * p[i]);
        pixel[i] = dd * m[0] + m[1 + i];
    }
}

// ortho.cpp:590-611 for one camera: in front of it (ray.z > 0) and projected inside its thumbnail
__device__ __forceinline__ bool thumbnail_pixel(const double *cam, double x, double y, double z, int *col, int *row)
{
    double ray[3];
    if (ochip_og::camera_ray_z(cam, x, y, z, ray) <= 0)
        return false;
    double pixel[2];
    camera_project(cam, ray, pixel);
    return ochip_og::thumbnail_cell(cam, pixel, col, row);
}

// computeDSMTile's per-pixel body: (float)z, NaN where no surface holds the pixel
__global__ __launch_bounds__(256) void ortho_dsm_kernel(mesh_args M, raster_args R, float *__restrict__ out,
                                                        uint32_t *__restrict__ tri_out, double *__restrict__ z64_out)
{
    int col;
    int64_t row;
    if (!tile_pixel(R, &col, &row))
        return;
    const double x = col * R.gsd + R.min_x;
    const double y = R.max_y - row * R.gsd;
    double z;
    const uint32_t t = mesh_height(M, x, y, R.mean_camera_z, &z);
    const size_t i = (size_t)(row - R.row0) * (size_t)R.cols + (size_t)col;
    out[i] = (float)z;
    if (tri_out)
        tri_out[i] = t;
    if (z64_out)
        z64_out[i] = z;
}

// generateOrthomosaic's per-pixel body (ortho.cpp:545-633).  cams [n][24]: position 3, R_inv 9 (row-major), f, ppx, ppy,
// k1, k2, k3, p1, p2, thumb_scale, thumbnail rows, thumbnail cols, unused.
__global__ __launch_bounds__(256) void ortho_thumbnail_kernel(mesh_args M, raster_args R, const double *__restrict__ cams,
                                                              uint32_t n_cams, const uint32_t *__restrict__ cam_id,
                                                              const uint64_t *__restrict__ thumb_off,
                                                              const uint8_t *__restrict__ thumbs, uint8_t *__restrict__ rgba,
                                                              uint32_t *__restrict__ ids, double *__restrict__ z_out,
                                                              uint32_t *__restrict__ tri_out)
{
    __shared__ double2 cam_xy[CAM_LDS_CHUNK];
    int col;
    int64_t row;
    const bool active = tile_pixel(R, &col, &row);
    const double x = col * R.gsd + R.min_x;
    const double y = R.max_y - row * R.gsd;
    // the 5 nearest cameras in XY
    double bd[KNN];
    uint32_t bi[KNN];
    for (int k = 0; k < KNN; k++)
        bd[k] = INFINITY, bi[k] = MISS;
    for (uint32_t base = 0; base < n_cams; base += CAM_LDS_CHUNK)
    {
        const uint32_t n = min(CAM_LDS_CHUNK, n_cams - base);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
            cam_xy[i] = make_double2(cams[(size_t)(base + i) * CAM_DOUBLES], cams[(size_t)(base + i) * CAM_DOUBLES + 1]);
        __syncthreads();
        for (uint32_t i = 0; i < n; i++)
        {
            const double2 c = cam_xy[i];
            const double dx = x - c.x, dy = y - c.y;
            ochip_og::knn_offer(dx * dx + dy * dy, base + i, bd, bi);
        }
    }
    if (!active)
        return;
    double z;
    const uint32_t t = mesh_height(M, x, y, R.mean_camera_z, &z);
    const size_t o = (size_t)(row - R.row0) * (size_t)R.cols + (size_t)col;
    if (z_out)
        z_out[o] = z;
    if (tri_out)
        tri_out[o] = t;
    uchar4 colour = make_uchar4(0, 0, 0, 0); // project-defined where no surface holds the pixel
    uint32_t source = MISS;
    if (t != MISS)
    {
        for (int k = 0; k < KNN && source == MISS; k++)
        {
            if (bi[k] == MISS)
                break;
            const double *c = cams + (size_t)bi[k] * CAM_DOUBLES;
            int tc, tr;
            if (!thumbnail_pixel(c, x, y, z, &tc, &tr))
                continue;
            const uint8_t *p = thumbs + thumb_off[bi[k]] + ((size_t)tr * (size_t)c[22] + tc) * 3;
            colour = make_uchar4(p[0], p[1], p[2], 255);
            source = cam_id[bi[k]];
        }
        if (source == MISS)
        {
            const uint8_t grey = (row + col) % 2 == 0 ? 64 : 128;
            colour = make_uchar4(grey, grey, grey, 0);
        }
    }
    reinterpret_cast<uchar4 *>(rgba)[o] = colour;
    ids[o] = source;
}

} // namespace

constexpr auto ENQ = ochip::copy_mode::enqueue; // uploads are enqueued on the context's stream; the caller waits

int ochip_ortho_mesh_create(ochip_ctx *ctx, uint32_t n_surfaces, const uint64_t *tri_off, const double *tri9,
                            ochip_ortho_mesh **out)
{
    if (!ctx || !out || !tri_off || (tri_off[n_surfaces] && !tri9))
        return ctx ? ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_mesh_create: bad argument") : OCHIP_EINVAL;
    if (tri_off[n_surfaces] >= MISS)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_mesh_create: too many triangles");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<ortho_surf> surf(n_surfaces);
    std::vector<uint32_t> cell_start, cell_tris;
    for (uint32_t s = 0; s < n_surfaces; s++)
    {
        const uint64_t t0 = tri_off[s], t1 = tri_off[s + 1];
        if (t1 < t0)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_mesh_create: tri_off is not ascending");
        double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
        for (uint64_t t = t0; t < t1; t++)
            for (int c = 0; c < 3; c++)
                for (int a = 0; a < 2; a++)
                {
                    const double v = tri9[9 * t + 3 * c + a];
                    if (!std::isfinite(v))
                        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_mesh_create: triangle %llu has a non-finite corner",
                                          (unsigned long long)t);
                    lo[a] = std::min(lo[a], v), hi[a] = std::max(hi[a], v);
                }
        ortho_surf &S = surf[s];
        S.cell_base = (uint32_t)cell_start.size();
        if (t1 == t0)
        {
            S.ox = S.oy = 0, S.cell = 1, S.ncx = S.ncy = 1;
            cell_start.push_back((uint32_t)cell_tris.size());
            cell_start.push_back((uint32_t)cell_tris.size());
            continue;
        }
        // about one cell per triangle, square cells, at most 4096 per side
        const double w = hi[0] - lo[0], h = hi[1] - lo[1];
        double cell = std::sqrt(std::max(w * h, 1e-300) / (double)(t1 - t0));
        cell = std::max({cell, w / 4096, h / 4096, 1e-9});
        S.ox = lo[0], S.oy = lo[1], S.cell = cell;
        S.ncx = std::max(1, std::min(4096, (int)std::ceil(w / cell)));
        S.ncy = std::max(1, std::min(4096, (int)std::ceil(h / cell)));
        std::vector<uint32_t> count((size_t)S.ncx * S.ncy + 1, 0);
        auto box = [&](uint64_t t, int *c0, int *c1) {
            double bl[2] = {INFINITY, INFINITY}, bh[2] = {-INFINITY, -INFINITY};
            for (int c = 0; c < 3; c++)
                for (int a = 0; a < 2; a++)
                    bl[a] = std::min(bl[a], tri9[9 * t + 3 * c + a]), bh[a] = std::max(bh[a], tri9[9 * t + 3 * c + a]);
            c0[0] = ochip_og::grid_cell(bl[0], S.ox, S.cell, S.ncx), c0[1] = ochip_og::grid_cell(bl[1], S.oy, S.cell, S.ncy);
            c1[0] = ochip_og::grid_cell(bh[0], S.ox, S.cell, S.ncx), c1[1] = ochip_og::grid_cell(bh[1], S.oy, S.cell, S.ncy);
        };
        for (uint64_t t = t0; t < t1; t++)
        {
            int c0[2], c1[2];
            box(t, c0, c1);
            for (int cy = c0[1]; cy <= c1[1]; cy++)
                for (int cx = c0[0]; cx <= c1[0]; cx++)
                    count[(size_t)cy * S.ncx + cx + 1]++;
        }
        for (size_t c = 1; c < count.size(); c++)
            count[c] += count[c - 1];
        const uint32_t base = (uint32_t)cell_tris.size();
        cell_tris.resize(base + (size_t)count.back());
        std::vector<uint32_t> fill(count.begin(), count.end() - 1);
        for (uint64_t t = t0; t < t1; t++) // ascending: every cell's list is sorted
        {
            int c0[2], c1[2];
            box(t, c0, c1);
            for (int cy = c0[1]; cy <= c1[1]; cy++)
                for (int cx = c0[0]; cx <= c1[0]; cx++)
                    cell_tris[base + fill[(size_t)cy * S.ncx + cx]++] = (uint32_t)t;
        }
        for (uint32_t c : count)
            cell_start.push_back(base + c);
    }
    ochip_ortho_mesh *m = new (std::nothrow) ochip_ortho_mesh();
    if (!m)
        return ochip_fail(ctx, OCHIP_ENOMEM, "out of host memory");
    m->ctx = m->mem.ctx = ctx;
    m->mem.what = "ochip_ortho_mesh_create";
    m->n_surfaces = n_surfaces;
    m->n_tris = (uint32_t)tri_off[n_surfaces];
    int rc = m->mem.upload(&m->surf, surf, ENQ);
    if (rc == OCHIP_OK)
        rc = m->mem.upload(&m->cell_start, cell_start, ENQ);
    if (rc == OCHIP_OK)
        rc = m->mem.upload(&m->cell_tris, cell_tris, ENQ);
    if (rc == OCHIP_OK)
        rc = m->mem.upload(&m->tris, tri9, (size_t)m->n_tris * 9, ENQ);
    if (rc == OCHIP_OK && ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        rc = ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ortho mesh)");
    if (rc != OCHIP_OK)
    {
        m->mem.release();
        delete m;
        return rc;
    }
    *out = m;
    return OCHIP_OK;
}

void ochip_ortho_mesh_destroy(ochip_ortho_mesh *m)
{
    if (!m)
        return;
    m->mem.release();
    delete m;
}

int ochip_ortho_dsm(ochip_ortho_mesh *m, const double *raster4, int32_t cols, int64_t row0, int64_t rows, float *out,
                    int out_on_device, uint32_t *tri_out, double *z64_out)
{
    if (!m || !raster4 || cols < 0 || row0 < 0 || rows < 0 || ((size_t)cols * rows && !out))
        return m ? ochip_fail(m->ctx, OCHIP_EINVAL, "ochip_ortho_dsm: bad argument") : OCHIP_EINVAL;
    ochip_ctx *ctx = m->ctx;
    if (cols == 0 || rows == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    // launches of at most ~2^26 pixels: bounded scratch for host outputs, and a grid of at most 2^18 workgroups
    const int64_t tile_rows = std::max<int64_t>(1, (int64_t)(((int64_t)1 << 26) / ((int64_t)cols * TILE)));
    const int64_t chunk = tile_rows * TILE;
    ochip::dev_scratch mem{ctx, "ochip_ortho_dsm"};
    float *dev_out = nullptr;
    uint32_t *dev_tri = nullptr;
    double *dev_z64 = nullptr;
    const size_t chunk_px = (size_t)std::min(chunk, rows) * cols;
    if (!out_on_device)
        OCHIP_TRY(mem.alloc<float>(&dev_out, chunk_px));
    if (tri_out)
        OCHIP_TRY(mem.alloc<uint32_t>(&dev_tri, chunk_px));
    if (z64_out)
        OCHIP_TRY(mem.alloc<double>(&dev_z64, chunk_px));
    for (int64_t r = 0; r < rows; r += chunk)
    {
        const int64_t n = std::min(chunk, rows - r);
        raster_args R = make_raster(raster4, cols, row0 + r, n);
        const uint32_t blocks_n = R.tiles_x * (uint32_t)((n + TILE - 1) / TILE);
        const size_t at = (size_t)r * cols, n_px = (size_t)n * cols;
        float *o = out_on_device ? out + at : dev_out;
        hipLaunchKernelGGL(ortho_dsm_kernel, dim3(blocks_n), dim3(TILE * TILE), 0, ctx->stream, m->args(), R, o, dev_tri, dev_z64);
        if (hipGetLastError() != hipSuccess)
            return ochip_fail(ctx, OCHIP_EHIP, "ortho_dsm_kernel launch failed");
        if (!out_on_device)
            OCHIP_TRY(copy_back(ctx, out + at, dev_out, n_px * sizeof(float), "DSM band"));
        if (tri_out)
            OCHIP_TRY(copy_back(ctx, tri_out + at, dev_tri, n_px * sizeof(uint32_t), "DSM triangles"));
        if (z64_out)
            OCHIP_TRY(copy_back(ctx, z64_out + at, dev_z64, n_px * sizeof(double), "DSM heights"));
        if ((!out_on_device || tri_out || z64_out) && ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
            return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (DSM band)");
    }
    // the scratch goes back to the pool only once nothing can still write it
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (DSM)");
    mem.release();
    return OCHIP_OK;
}

int ochip_ortho_thumbnail(ochip_ortho_mesh *m, const double *raster4, int32_t cols, int32_t rows, uint32_t n_cams,
                          const double *cams24, const uint32_t *cam_id, const uint64_t *thumb_off, const uint8_t *thumbs,
                          uint64_t thumb_bytes, uint8_t *rgba_out, uint32_t *id_out, double *z_out, uint32_t *tri_out)
{
    if (!m || !raster4 || cols < 0 || rows < 0 || (n_cams && (!cams24 || !cam_id || !thumb_off || !thumbs)) ||
        ((size_t)cols * rows && (!rgba_out || !id_out)))
        return m ? ochip_fail(m->ctx, OCHIP_EINVAL, "ochip_ortho_thumbnail: bad argument") : OCHIP_EINVAL;
    ochip_ctx *ctx = m->ctx;
    for (uint32_t i = 0; i < n_cams; i++) // every thumbnail read stays inside `thumbs`
    {
        const double *c = cams24 + (size_t)i * CAM_DOUBLES;
        if (!(c[21] >= 0 && c[21] < 65536 && c[22] >= 0 && c[22] < 65536) ||
            thumb_off[i] + (uint64_t)c[21] * (uint64_t)c[22] * 3 > thumb_bytes)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_thumbnail: camera %u's thumbnail lies outside the buffer", i);
    }
    const size_t px = (size_t)cols * rows;
    if (px == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_scratch mem{ctx, "ochip_ortho_thumbnail"};
    double *d_cams = nullptr, *d_z = nullptr;
    uint32_t *d_id = nullptr, *d_ids = nullptr, *d_tri = nullptr;
    uint64_t *d_off = nullptr;
    uint8_t *d_thumbs = nullptr, *d_rgba = nullptr;
    OCHIP_TRY(mem.upload(&d_cams, cams24, (size_t)n_cams * CAM_DOUBLES, ENQ));
    OCHIP_TRY(mem.upload(&d_id, cam_id, n_cams, ENQ));
    OCHIP_TRY(mem.upload(&d_off, thumb_off, n_cams, ENQ));
    OCHIP_TRY(mem.upload(&d_thumbs, thumbs, thumb_bytes, ENQ));
    OCHIP_TRY(mem.alloc<uint8_t>(&d_rgba, px * 4));
    OCHIP_TRY(mem.alloc<uint32_t>(&d_ids, px));
    if (z_out)
        OCHIP_TRY(mem.alloc<double>(&d_z, px));
    if (tri_out)
        OCHIP_TRY(mem.alloc<uint32_t>(&d_tri, px));
    raster_args R = make_raster(raster4, cols, 0, rows);
    const uint32_t blocks_n = R.tiles_x * (uint32_t)((rows + TILE - 1) / TILE);
    hipLaunchKernelGGL(ortho_thumbnail_kernel, dim3(blocks_n), dim3(TILE * TILE), 0, ctx->stream, m->args(), R, d_cams, n_cams, d_id,
                       d_off, d_thumbs, d_rgba, d_ids, d_z, d_tri);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "ortho_thumbnail_kernel launch failed");
    OCHIP_TRY(copy_back(ctx, rgba_out, d_rgba, px * 4, "thumbnail"));
    OCHIP_TRY(copy_back(ctx, id_out, d_ids, px * 4, "thumbnail"));
    OCHIP_TRY(copy_back(ctx, z_out, d_z, px * 8, "thumbnail"));
    OCHIP_TRY(copy_back(ctx, tri_out, d_tri, px * 4, "thumbnail"));
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (thumbnail)");
    mem.release();
    return OCHIP_OK;
}
