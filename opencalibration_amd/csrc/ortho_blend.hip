// libochip.so — the blended full-resolution orthomosaic (reference: blendLayeredGeoTIFF, src/ortho/ortho.cpp:1665-1990,
// and laplacianBlend, src/ortho/blending.cpp), one band of whole output tile rows per call.  The per-pixel and per-level
// rules are in ortho_blend.hpp, shared with the host's CPU route; this file lays them out over the band:
//
//   ortho_blend_prep      per pixel: validity, the recomputed weight, float Lab and its colour correction
//   ortho_blend_chamfer   per tile, one workgroup: the boundary mask and the 3 x 3 chamfer, row by row.  The forward pass
//                         of a row is the min over the three upper neighbours, e[c], then d[c] = min_j<=c e[j] + A (c - j),
//                         a prefix min of e[j] - A j plus A c; the backward pass mirrors it.  Exact in integers: it
//                         equals the sequential two-pass bit for bit.
//   ortho_blend_weights   per pixel: the falloff, the partition of unity, level 0 of the weight and colour x weight
//   ortho_blend_level     per (tile, level) pixel, one launch per level and step over all tiles of the band: the pull-push
//                         pyrDowns, the pull back up, the Gaussian pyrDowns, the blended Laplacian, the reconstruction
//   ortho_blend_final     per pixel: Lab -> BGR8 -> RGBA or the checkerboard
#include "ctx.hpp"
#include "ortho_blend.hpp"
#include "ortho_mesh.hpp"

#include <algorithm>
#include <vector>

using ochip_om::copy_back;

namespace
{

constexpr int THREADS = 256;
constexpr int SEG = ochip_ob::MAX_TILE / THREADS; // chamfer: columns per thread at most

__global__ __launch_bounds__(THREADS) void ortho_blend_prep(const ochip_ol::lab_tables *__restrict__ T, ochip_ob::band_view B,
                                                            const double *__restrict__ cams,
                                                            const ochip_ob::id_entry *__restrict__ ids, uint32_t n_ids,
                                                            ochip_ob::color_model0 M0)
{
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= B.rows * (int64_t)B.cols)
        return;
    ochip_ob::prep_pixel(*T, B, cams, ids, n_ids, M0, k / B.cols, (int32_t)(k % B.cols));
}

// inclusive scan (min) of one value per thread across the workgroup into lds[me], me = t (reverse: THREADS - 1 - t, a
// suffix min over the threads from t up)
__device__ __forceinline__ void block_min_scan(int32_t v, int32_t *lds, bool reverse)
{
    const int t = threadIdx.x;
    const int me = reverse ? THREADS - 1 - t : t;
    lds[me] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d *= 2)
    {
        const int32_t a = me >= d ? lds[me - d] : INT32_MAX;
        __syncthreads();
        lds[me] = min(lds[me], a);
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void ortho_blend_chamfer(ochip_ob::band_view B, const ochip_ob::tile_info *__restrict__ tiles)
{
    __shared__ int32_t prev[ochip_ob::MAX_TILE];
    __shared__ int32_t scan[THREADS];
    const ochip_ob::tile_info &t = tiles[blockIdx.x];
    const int tw = t.tw, th = t.th;
    const int per = (tw + THREADS - 1) / THREADS;
    const int c0 = threadIdx.x * per, c1 = min(c0 + per, tw); // this thread's columns [c0, c1)
    constexpr int32_t A = ochip_ob::CH_A, Bd = ochip_ob::CH_B;
    int32_t e[SEG];
    auto D = [&](int r, int c) -> int32_t * { return B.dist + (size_t)(t.r0 + r) * (size_t)B.cols + (size_t)(t.c0 + c); };
    for (int r = 0; r < th; r++)
    {
        int32_t run = INT32_MAX; // the thread's running min of e[j] - A j
        for (int c = c0; c < c1; c++)
        {
            int32_t v = ochip_ob::boundary_px(B, t, r, c) ? 0 : ochip_ob::DIST_INF;
            if (r > 0)
            {
                v = min(v, prev[c] + A);
                if (c > 0)
                    v = min(v, prev[c - 1] + Bd);
                if (c < tw - 1)
                    v = min(v, prev[c + 1] + Bd);
            }
            run = min(run, v - A * c);
            e[c - c0] = run;
        }
        block_min_scan(run, scan, false); // its barriers also close every thread's reads of the upper row
        const int32_t before = threadIdx.x > 0 ? scan[threadIdx.x - 1] : INT32_MAX;
        for (int c = c0; c < c1; c++)
        {
            const int32_t d = min(min(before, e[c - c0]) + A * c, ochip_ob::DIST_INF);
            prev[c] = d;
            *D(r, c) = d;
        }
        __syncthreads();
    }
    // backward, bottom row first; prev holds the row below
    for (int r = th - 1; r >= 0; r--)
    {
        int32_t run = INT32_MAX; // the thread's running min of e[j] + A j, from its last column down
        for (int c = c1 - 1; c >= c0; c--)
        {
            int32_t v = *D(r, c);
            if (r < th - 1)
            {
                v = min(v, prev[c] + A);
                if (c > 0)
                    v = min(v, prev[c - 1] + Bd);
                if (c < tw - 1)
                    v = min(v, prev[c + 1] + Bd);
            }
            run = min(run, v + A * c);
            e[c - c0] = run;
        }
        block_min_scan(run, scan, true);
        const int32_t after = threadIdx.x < THREADS - 1 ? scan[THREADS - 2 - threadIdx.x] : INT32_MAX;
        for (int c = c0; c < c1; c++)
        {
            const int32_t d = min(min(after, e[c - c0]) - A * c, ochip_ob::DIST_INF);
            prev[c] = d;
            *D(r, c) = d;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void ortho_blend_weights(ochip_ob::band_view B, ochip_ob::arena Ar,
                                                               const ochip_ob::tile_info *__restrict__ tiles, int T,
                                                               uint32_t tiles_x, float steepness)
{
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= B.rows * (int64_t)B.cols)
        return;
    const int64_t r = k / B.cols;
    const int32_t c = (int32_t)(k % B.cols);
    ochip_ob::weights_px(B, Ar, tiles[(size_t)(r / T) * tiles_x + (size_t)(c / T)], steepness, r, c);
}

enum step
{
    FILL_DOWN,
    FILL_UP,
    GAUSS_DOWN,
    BLEND,
    RECON
};

// blockIdx.y: tile (x layer for the per-layer steps); the tiles without this level return
__global__ __launch_bounds__(THREADS) void ortho_blend_level(ochip_ob::arena Ar, const ochip_ob::tile_info *__restrict__ tiles,
                                                             uint32_t n_tiles, int s, int lv)
{
    const uint32_t ti = blockIdx.y % n_tiles;
    const int l = (int)(blockIdx.y / n_tiles);
    const ochip_ob::tile_info &t = tiles[ti];
    const int levels = s == FILL_DOWN || s == FILL_UP ? t.lf : s == RECON ? t.p - 1 : t.p;
    if (lv >= levels)
        return;
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= (int64_t)t.lw[lv] * t.lh[lv])
        return;
    const int x = (int)(k % t.lw[lv]), y = (int)(k / t.lw[lv]);
    switch (s)
    {
    case FILL_DOWN:
        ochip_ob::fill_down_px(Ar, t, l, lv, x, y);
        break;
    case FILL_UP:
        ochip_ob::fill_up_px(Ar, t, l, lv, x, y);
        break;
    case GAUSS_DOWN:
        ochip_ob::gauss_down_px(Ar, t, l, lv, x, y);
        break;
    case BLEND:
        ochip_ob::blend_px(Ar, t, lv, x, y);
        break;
    default:
        ochip_ob::recon_px(Ar, t, lv, x, y);
    }
}

__global__ __launch_bounds__(THREADS) void ortho_blend_final(const ochip_ol::lab_tables *__restrict__ T, ochip_ob::band_view B,
                                                             ochip_ob::arena Ar, const ochip_ob::tile_info *__restrict__ tiles,
                                                             int TS, uint32_t tiles_x, uint8_t *__restrict__ rgba)
{
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= B.rows * (int64_t)B.cols)
        return;
    const int64_t r = k / B.cols;
    const int32_t c = (int32_t)(k % B.cols);
    ochip_ob::final_px(*T, B, Ar, tiles[(size_t)(r / TS) * tiles_x + (size_t)(c / TS)], r, c, rgba);
}

// laplacianBlend alone on one tile (ochip_laplacian_blend): the given layers and weights seed level 0
__global__ __launch_bounds__(THREADS) void ortho_blend_seed(ochip_ob::arena Ar, int64_t px, const float *__restrict__ lab,
                                                            const float *__restrict__ weight)
{
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= px)
        return;
    float w[ochip_ob::MAX_LAYERS];
    for (int l = 0; l < Ar.L; l++)
        w[l] = weight[(size_t)l * px + k];
    ochip_ob::unity_px(Ar, k, w, lab + 3 * k, 3 * (size_t)px);
}

__global__ __launch_bounds__(THREADS) void ortho_blend_seed_out(const ochip_ol::lab_tables *__restrict__ T, ochip_ob::arena Ar,
                                                                int64_t px, uint8_t *__restrict__ bgra)
{
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= px)
        return;
    ochip_ob::blended_bgr8(*T, Ar, k, bgra + 4 * k);
    bgra[4 * k + 3] = 255;
}

// the pyramid steps of laplacianBlend over every tile of `tiles` (uploaded at d_tiles), on the context's stream
void blend_levels(hipStream_t st, const ochip_ob::arena &Ar, const std::vector<ochip_ob::tile_info> &tiles,
                  const ochip_ob::tile_info *d_tiles)
{
    const uint32_t n_tiles = (uint32_t)tiles.size();
    int max_lf = 0, max_p = 0;
    for (const auto &t : tiles)
        max_lf = std::max(max_lf, t.lf), max_p = std::max(max_p, t.p);
    // the largest tile's level lv sets the grid of a level launch
    auto level = [&](int s, int lv, uint32_t layers) {
        int64_t most = 0;
        for (const auto &t : tiles)
            if (lv < t.lf)
                most = std::max<int64_t>(most, (int64_t)t.lw[lv] * t.lh[lv]);
        if (most)
            hipLaunchKernelGGL(ortho_blend_level, dim3((uint32_t)((most + THREADS - 1) / THREADS), n_tiles * layers),
                               dim3(THREADS), 0, st, Ar, d_tiles, n_tiles, s, lv);
    };
    for (int lv = 1; lv < max_lf; lv++)
        level(FILL_DOWN, lv, Ar.L);
    for (int lv = max_lf - 1; lv >= 0; lv--)
        level(FILL_UP, lv, Ar.L);
    for (int lv = 1; lv < max_p; lv++)
        level(GAUSS_DOWN, lv, Ar.L);
    for (int lv = 0; lv < max_p; lv++)
        level(BLEND, lv, 1);
    for (int lv = max_p - 2; lv >= 0; lv--)
        level(RECON, lv, 1);
}

constexpr auto ENQ = ochip::copy_mode::enqueue; // uploads are enqueued on the context's stream; the caller waits

int arena_alloc(ochip::dev_blocks &mem, ochip_ob::arena *Ar)
{
    const size_t n = (size_t)Ar->n, L = (size_t)Ar->L;
    OCHIP_TRY(mem.alloc(&Ar->wr, L * n));
    OCHIP_TRY(mem.alloc(&Ar->wc, L * n * 3));
    OCHIP_TRY(mem.alloc(&Ar->fl, L * n * 3));
    OCHIP_TRY(mem.alloc(&Ar->g, L * n * 3));
    return mem.alloc(&Ar->bl, n * 3);
}

} // namespace

int ochip_laplacian_blend(ochip_ctx *ctx, int32_t num_layers, int32_t rows, int32_t cols, int32_t pyramid_levels,
                          const float *lab, const float *weight, uint8_t *bgra_out)
{
    if (!ctx || num_layers < 1 || num_layers > ochip_ob::MAX_LAYERS || rows < 0 || cols < 0 || rows > ochip_ob::MAX_TILE ||
        cols > ochip_ob::MAX_TILE || ((size_t)rows * cols && (!lab || !weight || !bgra_out)))
        return ctx ? ochip_fail(ctx, OCHIP_EINVAL, "ochip_laplacian_blend: 1..%d layers of at most %d x %d",
                                ochip_ob::MAX_LAYERS, ochip_ob::MAX_TILE, ochip_ob::MAX_TILE)
                   : OCHIP_EINVAL;
    const size_t px = (size_t)rows * (size_t)cols;
    if (px == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip_ol::lab_tables tables;
    ochip_ol::lab_tables_build(&tables);
    std::vector<ochip_ob::tile_info> tiles;
    ochip_ob::arena Ar{num_layers, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    Ar.n = ochip_ob::tiles_build(std::max(rows, cols), rows, cols, pyramid_levels, &tiles);
    ochip::dev_scratch mem{ctx, "ochip_laplacian_blend"};
    float *d_lab = nullptr, *d_w = nullptr;
    uint8_t *d_out = nullptr;
    ochip_ol::lab_tables *d_tab = nullptr;
    ochip_ob::tile_info *d_tiles = nullptr;
    OCHIP_TRY(mem.upload<ochip_ol::lab_tables>(&d_tab, &tables, 1, ENQ));
    OCHIP_TRY(mem.upload(&d_tiles, tiles, ENQ));
    OCHIP_TRY(mem.upload(&d_lab, lab, (size_t)num_layers * px * 3, ENQ));
    OCHIP_TRY(mem.upload(&d_w, weight, (size_t)num_layers * px, ENQ));
    OCHIP_TRY(mem.alloc(&d_out, px * 4));
    OCHIP_TRY(arena_alloc(mem, &Ar));
    const uint32_t grid = (uint32_t)((px + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(ortho_blend_seed, dim3(grid), dim3(THREADS), 0, ctx->stream, Ar, (int64_t)px, d_lab, d_w);
    blend_levels(ctx->stream, Ar, tiles, d_tiles);
    hipLaunchKernelGGL(ortho_blend_seed_out, dim3(grid), dim3(THREADS), 0, ctx->stream, d_tab, Ar, (int64_t)px, d_out);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "laplacian_blend kernel launch failed");
    OCHIP_TRY(copy_back(ctx, bgra_out, d_out, px * 4, "laplacian blend"));
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (laplacian blend)");
    mem.release();
    return OCHIP_OK;
}

int ochip_ortho_blend(ochip_ctx *ctx, const double *raster3, int32_t cols, int64_t row0, int64_t rows, const int32_t *config4,
                      uint32_t n_cams, const double *cams, uint32_t n_ids, const ochip_blend_id *ids, const double *vig0,
                      int on_device, const uint8_t *bgra, const uint64_t *id, const float *dsm, uint8_t *rgba_out,
                      float *weight_out, float *dist_out, float *lab_out)
{
    static_assert(sizeof(ochip_blend_id) == sizeof(ochip_ob::id_entry), "ochip_blend_id layout");
    if (!ctx || !raster3 || !config4 || cols < 0 || row0 < 0 || rows < 0 || (n_cams && !cams) || (n_ids && !ids) ||
        ((size_t)cols * rows && (!bgra || !id || !dsm || !rgba_out)))
        return ctx ? ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_blend: bad argument") : OCHIP_EINVAL;
    const int L = config4[0], TS = config4[1], P = config4[2], radius = config4[3];
    if (L < 1 || L > ochip_ob::MAX_LAYERS || TS < 1 || TS > ochip_ob::MAX_TILE || radius < 1 || row0 % TS != 0)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_blend: num_layers 1..%d, tile_size 1..%d, "
                                             "blend_transition_radius >= 1 and a band that starts on a tile row",
                          ochip_ob::MAX_LAYERS, ochip_ob::MAX_TILE);
    for (uint32_t i = 0; i < n_ids; i++)
        if ((i && ids[i].id <= ids[i - 1].id) || (ids[i].cam != ochip_ob::NONE && ids[i].cam >= n_cams))
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_blend: ids must be sorted, unique and name cameras < n_cams");
    const size_t px = (size_t)cols * (size_t)rows;
    if (px == 0)
        return OCHIP_OK;
    if ((uint64_t)((rows + TS - 1) / TS) * (uint64_t)((cols + TS - 1) / TS) * (uint64_t)L > 65535)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_blend: more than 65535 tiles x layers in one band");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip_ol::lab_tables tables;
    ochip_ol::lab_tables_build(&tables);
    std::vector<ochip_ob::tile_info> tiles;
    const int64_t n = ochip_ob::tiles_build(TS, rows, cols, P, &tiles);
    const uint32_t n_tiles = (uint32_t)tiles.size(), tiles_x = (uint32_t)((cols + TS - 1) / TS);
    const float steepness = (float)std::log(99.0) / (float)radius;
    const ochip_ob::color_model0 M0{vig0 ? 1 : 0, {vig0 ? vig0[0] : 0, vig0 ? vig0[1] : 0, vig0 ? vig0[2] : 0}};

    const size_t Lpx = (size_t)L * px;
    std::vector<int32_t> dist(dist_out ? px : 0); // (outlives the blocks: a copy into it may be in flight on an early return)
    ochip::dev_scratch mem{ctx, "ochip_ortho_blend"};
    double *d_cams = nullptr;
    ochip_ob::id_entry *d_ids = nullptr;
    ochip_ol::lab_tables *d_lab = nullptr;
    ochip_ob::tile_info *d_tiles = nullptr;
    uint8_t *d_bgra = nullptr, *d_valid = nullptr, *d_rgba = nullptr;
    uint64_t *d_id = nullptr;
    float *d_dsm = nullptr, *d_weight = nullptr, *d_labp = nullptr;
    int32_t *d_dist = nullptr;
    ochip_ob::arena Ar{L, n, nullptr, nullptr, nullptr, nullptr, nullptr};
    OCHIP_TRY(mem.upload(&d_cams, cams, (size_t)n_cams * ochip_ol::CAM_DOUBLES, ENQ));
    OCHIP_TRY(mem.upload(&d_ids, (const ochip_ob::id_entry *)ids, n_ids, ENQ));
    OCHIP_TRY(mem.upload<ochip_ol::lab_tables>(&d_lab, &tables, 1, ENQ));
    OCHIP_TRY(mem.upload(&d_tiles, tiles, ENQ));
    if (!on_device)
    {
        OCHIP_TRY(mem.upload(&d_bgra, bgra, Lpx * 4, ENQ));
        OCHIP_TRY(mem.upload(&d_id, id, Lpx, ENQ));
        OCHIP_TRY(mem.upload(&d_dsm, dsm, px, ENQ));
        OCHIP_TRY(mem.alloc(&d_rgba, px * 4));
    }
    OCHIP_TRY(mem.alloc(&d_valid, Lpx));
    OCHIP_TRY(mem.alloc(&d_weight, Lpx));
    OCHIP_TRY(mem.alloc(&d_labp, Lpx * 3));
    OCHIP_TRY(mem.alloc(&d_dist, px));
    OCHIP_TRY(arena_alloc(mem, &Ar));
    ochip_ob::band_view B{L,
                          cols,
                          rows,
                          row0,
                          raster3[0],
                          raster3[1],
                          raster3[2],
                          on_device ? bgra : d_bgra,
                          on_device ? id : d_id,
                          on_device ? dsm : d_dsm,
                          d_valid,
                          d_weight,
                          d_labp,
                          d_dist};
    uint8_t *rgba = on_device ? rgba_out : d_rgba;
    const uint32_t grid = (uint32_t)((px + THREADS - 1) / THREADS);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(ortho_blend_prep, dim3(grid), dim3(THREADS), 0, st, d_lab, B, d_cams, d_ids, n_ids, M0);
    hipLaunchKernelGGL(ortho_blend_chamfer, dim3(n_tiles), dim3(THREADS), 0, st, B, d_tiles);
    hipLaunchKernelGGL(ortho_blend_weights, dim3(grid), dim3(THREADS), 0, st, B, Ar, d_tiles, TS, tiles_x, steepness);
    blend_levels(st, Ar, tiles, d_tiles);
    hipLaunchKernelGGL(ortho_blend_final, dim3(grid), dim3(THREADS), 0, st, d_lab, B, Ar, d_tiles, TS, tiles_x, rgba);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "ortho_blend kernel launch failed");
    const char *what = "ortho blend";
    if (!on_device)
        OCHIP_TRY(copy_back(ctx, rgba_out, d_rgba, px * 4, what));
    OCHIP_TRY(copy_back(ctx, weight_out, d_weight, Lpx * 4, what));
    OCHIP_TRY(copy_back(ctx, lab_out, d_labp, Lpx * 12, what));
    OCHIP_TRY(copy_back(ctx, dist_out ? dist.data() : nullptr, d_dist, px * 4, what));
    if (ochip_stream_wait(ctx, st) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ortho blend)");
    mem.release();
    if (dist_out)
        for (size_t i = 0; i < px; i++)
            dist_out[i] = ochip_ob::dist_float(dist[i]);
    return OCHIP_OK;
}
