// libochip.so — the layered full-resolution orthomosaic (reference: generateLayeredGeoTIFF / processLayeredTile,
// src/ortho/ortho.cpp:1206-1663), one band of whole output tile rows per call.  The per-pixel rules are in
// ortho_layers.hpp, shared with the host's CPU route; this file does what only the device does:
//
// Pass 1 (ortho_layers_pass1): 16 x 16 pixel tiles per workgroup (as ortho.hip).  The workgroup first builds the exact
// kNN candidate list of its rectangle: thr = the 5th smallest *farthest* squared distance from a camera to the rectangle,
// candidates = every camera whose *nearest* squared distance is <= thr, in ascending camera order, staged in LDS.  A pixel's
// 5 nearest cameras are all candidates (5 cameras lie within thr of it; a non-candidate lies beyond thr), and the
// rectangle's corners are pixel centres computed with the pixels' own expressions, so the rounded distances keep the order
// and the pruned search equals brute force, ties included.  Then per pixel: the mesh height (ortho_mesh.hpp), (float)z,
// and the layers of up to num_layers cameras (ortho_layers.hpp: pixel_layers).
//
// Pass 2 on the finished band: ortho_layers_count gives every pixel its record count in the canonical order (output tiles
// row-major, then local raster order), ortho_layers_block_sums / ortho_layers_scan_top an exclusive scan of the counts,
// and ortho_layers_write the records at their offsets, (a, b) lexicographically.  No sort: the order is the scan's.
#include "ctx.hpp"
#include "ortho_layers.hpp"
#include "ortho_mesh.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace ochip_om;

namespace
{

constexpr int THREADS = TILE * TILE; // a pass-1 workgroup's tile
constexpr uint32_t CAND_CAP = 1024; // kNN candidates staged in LDS; a tile with more scans every camera
constexpr int ITEMS = 16;           // pass-2 scan: counts per thread
constexpr int CHUNK = THREADS * ITEMS;
constexpr int KNN = ochip_ol::KNN;

// the 5 smallest of two sorted lists of 5, sorted
__device__ __forceinline__ void merge5(const double *a, const double *b, double *out)
{
    int i = 0, j = 0;
    double m[KNN];
    for (int k = 0; k < KNN; k++)
        m[k] = (j >= KNN || (i < KNN && a[i] <= b[j])) ? a[i++] : b[j++];
    for (int k = 0; k < KNN; k++)
        out[k] = m[k];
}

__global__ __launch_bounds__(THREADS) void ortho_layers_pass1(mesh_args M, raster_args R, const double *__restrict__ cams,
                                                              uint32_t n_cams, const uint8_t *const *__restrict__ images,
                                                              const uint64_t *__restrict__ node_ids,
                                                              const ochip_ol::lab_tables *__restrict__ lab,
                                                              ochip_ol::band_planes B, uint32_t *__restrict__ knn_out)
{
    __shared__ double2 cand_xy[CAND_CAP];
    __shared__ uint32_t cand_id[CAND_CAP];
    __shared__ double far5[THREADS][KNN];
    __shared__ uint32_t wave_count[THREADS / 64];
    __shared__ uint32_t n_cand;
    const uint32_t t = threadIdx.x;
    const uint32_t tx = blockIdx.x % R.tiles_x, ty = blockIdx.x / R.tiles_x;
    const int c_lo = (int)(tx * TILE), c_hi = min(c_lo + TILE, R.cols) - 1;
    const int64_t lr_lo = (int64_t)ty * TILE, lr_hi = min<int64_t>(lr_lo + TILE, R.rows) - 1;
    // the rectangle of pixel centres, with the pixels' own expressions
    const double x_lo = c_lo * R.gsd + R.min_x, x_hi = c_hi * R.gsd + R.min_x;
    const double y_hi = R.max_y - (R.row0 + lr_lo) * R.gsd, y_lo = R.max_y - (R.row0 + lr_hi) * R.gsd;

    // thr: the 5th smallest farthest distance
    double mine[KNN];
    for (int k = 0; k < KNN; k++)
        mine[k] = INFINITY;
    for (uint32_t i = t; i < n_cams; i += THREADS)
    {
        const double cx = cams[(size_t)i * ochip_ol::CAM_DOUBLES], cy = cams[(size_t)i * ochip_ol::CAM_DOUBLES + 1];
        const double ax = x_lo - cx, bx = x_hi - cx, ay = y_lo - cy, by = y_hi - cy;
        double d = fmax(ax * ax, bx * bx) + fmax(ay * ay, by * by);
        for (int k = 0; k < KNN; k++) // insertion into the sorted list
            if (d < mine[k])
            {
                const double s = mine[k];
                mine[k] = d;
                d = s;
            }
    }
    for (int k = 0; k < KNN; k++)
        far5[t][k] = mine[k];
    for (uint32_t half = THREADS / 2; half > 0; half /= 2)
    {
        __syncthreads();
        if (t < half)
        {
            double m[KNN];
            merge5(far5[t], far5[t + half], m);
            for (int k = 0; k < KNN; k++)
                far5[t][k] = m[k];
        }
    }
    if (t == 0)
        n_cand = 0;
    __syncthreads();
    const double thr = far5[0][KNN - 1];

    // the candidates in ascending order: a ballot per wavefront and chunk
    const uint32_t lane = t % 64, wave = t / 64;
    for (uint32_t base = 0; base < n_cams; base += THREADS)
    {
        const uint32_t i = base + t;
        bool keep = false;
        double cx = 0, cy = 0;
        if (i < n_cams)
        {
            cx = cams[(size_t)i * ochip_ol::CAM_DOUBLES], cy = cams[(size_t)i * ochip_ol::CAM_DOUBLES + 1];
            const double dx = cx < x_lo ? x_lo - cx : cx > x_hi ? x_hi - cx : 0.0;
            const double dy = cy < y_lo ? y_lo - cy : cy > y_hi ? y_hi - cy : 0.0;
            keep = dx * dx + dy * dy <= thr;
        }
        const uint64_t ballot = __ballot(keep);
        if (lane == 0)
            wave_count[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t off = n_cand;
        for (uint32_t w = 0; w < wave; w++)
            off += wave_count[w];
        off += (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        if (keep && off < CAND_CAP)
        {
            cand_xy[off] = make_double2(cx, cy);
            cand_id[off] = i;
        }
        __syncthreads();
        if (t == 0)
            for (uint32_t w = 0; w < THREADS / 64; w++)
                n_cand += wave_count[w];
        __syncthreads();
    }

    const int col = c_lo + (int)(t % TILE);
    const int64_t lr = lr_lo + t / TILE;
    if (col > c_hi || lr > lr_hi)
        return;
    const int64_t row = R.row0 + lr;
    const double x = col * R.gsd + R.min_x;
    const double y = R.max_y - row * R.gsd;
    double bd[KNN];
    uint32_t bi[KNN];
    for (int k = 0; k < KNN; k++)
        bd[k] = INFINITY, bi[k] = ochip_ol::NONE;
    if (n_cand <= CAND_CAP)
        for (uint32_t k = 0; k < n_cand; k++)
        {
            const double2 c = cand_xy[k];
            const double dx = x - c.x, dy = y - c.y;
            ochip_og::knn_offer(dx * dx + dy * dy, cand_id[k], bd, bi);
        }
    else
        for (uint32_t i = 0; i < n_cams; i++)
        {
            const double dx = x - cams[(size_t)i * ochip_ol::CAM_DOUBLES], dy = y - cams[(size_t)i * ochip_ol::CAM_DOUBLES + 1];
            ochip_og::knn_offer(dx * dx + dy * dy, i, bd, bi);
        }
    const size_t o = (size_t)lr * (size_t)R.cols + (size_t)col;
    if (knn_out)
        for (int k = 0; k < KNN; k++)
            knn_out[o * KNN + k] = bi[k];
    double z;
    mesh_height(M, x, y, R.mean_camera_z, &z);
    const ochip_ol::cameras_view C{cams, images, n_cams};
    ochip_ol::pixel_layers(*lab, C, node_ids, bi, x, y, (float)z, R.gsd, B, o);
}

// The front half of ortho_layers_pass1 alone, over every band of a raster in one launch: the tile's exact candidate list, each
// pixel's kNN, and a byte per (band, camera) that some pixel of the band has among its 5 nearest.  A workgroup's tile lies
// inside one band (blockIdx.y), so a band whose height is no multiple of TILE ends on a partial tile of its own.  The kNN
// runs over positions in the candidate list (ascending camera order, so the tie order is the cameras'); the members are
// flagged in LDS and one lane per flagged candidate stores the byte.  Every writer stores the same value: plain stores.
// This repeats pass 1's candidate-list code instead of sharing it, so that kernel's code object stays what was measured.
__global__ __launch_bounds__(THREADS) void ortho_band_cameras_kernel(raster_args R, int64_t band_rows, uint32_t tiles_per_band_y,
                                                                     const double *__restrict__ cams, uint32_t n_cams,
                                                                     uint8_t *__restrict__ used)
{
    __shared__ double2 cand_xy[CAND_CAP];
    __shared__ uint32_t cand_id[CAND_CAP];
    __shared__ uint8_t cand_flag[CAND_CAP];
    __shared__ double far5[THREADS][KNN];
    __shared__ uint32_t wave_count[THREADS / 64];
    __shared__ uint32_t n_cand;
    const uint32_t t = threadIdx.x;
    const uint32_t tx = blockIdx.x;
    const uint32_t band = blockIdx.y / tiles_per_band_y, ty = blockIdx.y % tiles_per_band_y;
    const int c_lo = (int)(tx * TILE), c_hi = min(c_lo + TILE, R.cols) - 1;
    const int64_t band_lo = (int64_t)band * band_rows, band_hi = min<int64_t>(band_lo + band_rows, R.rows);
    const int64_t lr_lo = band_lo + (int64_t)ty * TILE, lr_hi = min<int64_t>(lr_lo + TILE, band_hi) - 1;
    if (lr_lo > lr_hi) // the raster's last band may be shorter than the others: the whole workgroup leaves
        return;
    const double x_lo = c_lo * R.gsd + R.min_x, x_hi = c_hi * R.gsd + R.min_x;
    const double y_hi = R.max_y - lr_lo * R.gsd, y_lo = R.max_y - lr_hi * R.gsd;

    double mine[KNN];
    for (int k = 0; k < KNN; k++)
        mine[k] = INFINITY;
    for (uint32_t i = t; i < n_cams; i += THREADS)
    {
        const double cx = cams[(size_t)i * ochip_ol::CAM_DOUBLES], cy = cams[(size_t)i * ochip_ol::CAM_DOUBLES + 1];
        const double ax = x_lo - cx, bx = x_hi - cx, ay = y_lo - cy, by = y_hi - cy;
        double d = fmax(ax * ax, bx * bx) + fmax(ay * ay, by * by);
        for (int k = 0; k < KNN; k++)
            if (d < mine[k])
            {
                const double s = mine[k];
                mine[k] = d;
                d = s;
            }
    }
    for (int k = 0; k < KNN; k++)
        far5[t][k] = mine[k];
    for (uint32_t half = THREADS / 2; half > 0; half /= 2)
    {
        __syncthreads();
        if (t < half)
        {
            double m[KNN];
            merge5(far5[t], far5[t + half], m);
            for (int k = 0; k < KNN; k++)
                far5[t][k] = m[k];
        }
    }
    if (t == 0)
        n_cand = 0;
    for (uint32_t k = t; k < CAND_CAP; k += THREADS)
        cand_flag[k] = 0;
    __syncthreads();
    const double thr = far5[0][KNN - 1];

    const uint32_t lane = t % 64, wave = t / 64;
    for (uint32_t base = 0; base < n_cams; base += THREADS)
    {
        const uint32_t i = base + t;
        bool keep = false;
        double cx = 0, cy = 0;
        if (i < n_cams)
        {
            cx = cams[(size_t)i * ochip_ol::CAM_DOUBLES], cy = cams[(size_t)i * ochip_ol::CAM_DOUBLES + 1];
            const double dx = cx < x_lo ? x_lo - cx : cx > x_hi ? x_hi - cx : 0.0;
            const double dy = cy < y_lo ? y_lo - cy : cy > y_hi ? y_hi - cy : 0.0;
            keep = dx * dx + dy * dy <= thr;
        }
        const uint64_t ballot = __ballot(keep);
        if (lane == 0)
            wave_count[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t off = n_cand;
        for (uint32_t w = 0; w < wave; w++)
            off += wave_count[w];
        off += (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        if (keep && off < CAND_CAP)
        {
            cand_xy[off] = make_double2(cx, cy);
            cand_id[off] = i;
        }
        __syncthreads();
        if (t == 0)
            for (uint32_t w = 0; w < THREADS / 64; w++)
                n_cand += wave_count[w];
        __syncthreads();
    }

    const int col = c_lo + (int)(t % TILE);
    const int64_t row = lr_lo + t / TILE;
    const bool listed = n_cand <= CAND_CAP; // uniform over the workgroup
    uint8_t *mine_used = used + (size_t)band * n_cams;
    if (col <= c_hi && row <= lr_hi)
    {
        const double x = col * R.gsd + R.min_x;
        const double y = R.max_y - row * R.gsd;
        double bd[KNN];
        uint32_t bi[KNN];
        for (int k = 0; k < KNN; k++)
            bd[k] = INFINITY, bi[k] = ochip_ol::NONE;
        if (listed)
            for (uint32_t k = 0; k < n_cand; k++)
            {
                const double2 c = cand_xy[k];
                const double dx = x - c.x, dy = y - c.y;
                ochip_og::knn_offer(dx * dx + dy * dy, k, bd, bi);
            }
        else
            for (uint32_t i = 0; i < n_cams; i++)
            {
                const double dx = x - cams[(size_t)i * ochip_ol::CAM_DOUBLES], dy = y - cams[(size_t)i * ochip_ol::CAM_DOUBLES + 1];
                ochip_og::knn_offer(dx * dx + dy * dy, i, bd, bi);
            }
        for (int k = 0; k < KNN; k++)
            if (bi[k] != ochip_ol::NONE) // fewer than 5 cameras: the padding names no table entry
            {
                if (listed)
                    cand_flag[bi[k]] = 1;
                else
                    mine_used[bi[k]] = 1;
            }
    }
    __syncthreads();
    if (listed)
        for (uint32_t k = t; k < n_cand; k += THREADS)
            if (cand_flag[k])
                mine_used[cand_id[k]] = 1;
}

// canonical index k of the band -> band-local (r, c): output tiles row-major, then local raster order
__device__ __forceinline__ void canon_pixel(int64_t k, int T, int32_t W, int64_t rows, int64_t *r, int32_t *c)
{
    const int64_t per_tile_row = (int64_t)T * W;
    const int64_t ty = k / per_tile_row, r0 = ty * T;
    const int64_t th = min<int64_t>(T, rows - r0);
    const int64_t rem = k - ty * per_tile_row;
    const int64_t tx = rem / ((int64_t)T * th), c0 = tx * T;
    const int64_t tw = min<int64_t>(T, W - c0);
    const int64_t rem2 = rem - tx * T * th;
    *r = r0 + rem2 / tw;
    *c = (int32_t)(c0 + rem2 % tw);
}

__global__ __launch_bounds__(THREADS) void ortho_layers_count(ochip_ol::band_planes B, ochip_ol::corr_config K,
                                                              uint8_t *__restrict__ counts)
{
    const int64_t px = B.rows * (int64_t)B.cols;
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= px)
        return;
    int64_t r;
    int32_t c;
    canon_pixel(k, K.tile_size, B.cols, B.rows, &r, &c);
    counts[k] = (uint8_t)ochip_ol::corr_count(B, K, r, c);
}

// the block's exclusive prefix of its threads' ITEMS counts (LDS scan), and the block's total
__device__ __forceinline__ uint64_t block_prefix(uint64_t v, uint64_t *lds, uint64_t *total)
{
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d *= 2)
    {
        const uint64_t a = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += a;
        __syncthreads();
    }
    const uint64_t incl = lds[t];
    *total = lds[THREADS - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ uint64_t thread_sum(const uint8_t *counts, int64_t px, int64_t first)
{
    uint64_t s = 0;
    for (int j = 0; j < ITEMS; j++)
        if (first + j < px)
            s += counts[first + j];
    return s;
}

__global__ __launch_bounds__(THREADS) void ortho_layers_block_sums(const uint8_t *__restrict__ counts, int64_t px,
                                                                   uint64_t *__restrict__ bsum)
{
    __shared__ uint64_t lds[THREADS];
    const int64_t first = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * ITEMS;
    uint64_t total;
    block_prefix(thread_sum(counts, px, first), lds, &total);
    if (threadIdx.x == 0)
        bsum[blockIdx.x] = total;
}

// one workgroup: bsum -> its exclusive prefix; *grand = the sum
__global__ __launch_bounds__(THREADS) void ortho_layers_scan_top(uint64_t *__restrict__ bsum, uint32_t nb,
                                                                 uint64_t *__restrict__ grand)
{
    __shared__ uint64_t lds[THREADS];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += THREADS)
    {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? bsum[i] : 0;
        uint64_t total;
        const uint64_t ex = block_prefix(v, lds, &total);
        if (i < nb)
            bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0)
        *grand = carry;
}

__global__ __launch_bounds__(THREADS) void ortho_layers_write(const ochip_ol::lab_tables *__restrict__ lab,
                                                              ochip_ol::band_planes B, ochip_ol::corr_config K,
                                                              const uint32_t *__restrict__ model_ids,
                                                              const uint8_t *__restrict__ counts,
                                                              const uint64_t *__restrict__ bsum,
                                                              ochip_ol::corr_record *__restrict__ out, uint64_t capacity)
{
    __shared__ uint64_t lds[THREADS];
    const int64_t px = B.rows * (int64_t)B.cols;
    const int64_t first = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * ITEMS;
    uint64_t total;
    uint64_t off = bsum[blockIdx.x] + block_prefix(thread_sum(counts, px, first), lds, &total);
    for (int j = 0; j < ITEMS && first + j < px; j++)
    {
        const uint32_t n = counts[first + j];
        if (n == 0)
            continue;
        if (off + n <= capacity)
        {
            int64_t r;
            int32_t c;
            canon_pixel(first + j, K.tile_size, B.cols, B.rows, &r, &c);
            ochip_ol::corr_write(*lab, B, K, model_ids, r, c, out + off);
        }
        off += n;
    }
}

} // namespace

int ochip_ortho_layers(ochip_ortho_mesh *m, const double *raster4, int32_t cols, int64_t row0, int64_t rows,
                       const int32_t *config4, uint32_t n_cams, const double *cams, const uint64_t *node_ids,
                       const uint32_t *model_ids, const uint64_t *images, int out_on_device, uint8_t *bgra_out,
                       uint64_t *id_out, float *weight_out, ochip_color_corr *corr_out, uint64_t corr_capacity,
                       uint64_t *n_corr, uint32_t *knn_out)
{
    static_assert(sizeof(ochip_color_corr) == sizeof(ochip_ol::corr_record), "ochip_color_corr layout");
    if (!m || !raster4 || !config4 || cols < 0 || row0 < 0 || rows < 0 || !n_corr ||
        (n_cams && (!cams || !node_ids || !model_ids || !images)) || ((size_t)cols * rows && (!bgra_out || !id_out)) ||
        (corr_capacity && !corr_out))
        return m ? ochip_fail(m->ctx, OCHIP_EINVAL, "ochip_ortho_layers: bad argument") : OCHIP_EINVAL;
    ochip_ctx *ctx = m->ctx;
    const int L = config4[0], T = config4[1];
    const ochip_ol::corr_config K{T, config4[2], config4[3], row0};
    if (L < 1 || L > ochip_ol::MAX_LAYERS || T < 1 || K.radius < 0 || row0 % T != 0)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_layers: num_layers 1..%d, tile_size >= 1, radius >= 0 and a band "
                                             "that starts on a tile row", ochip_ol::MAX_LAYERS);
    for (uint32_t i = 0; i < n_cams; i++)
    {
        const double *c = cams + (size_t)i * ochip_ol::CAM_DOUBLES;
        if (!(c[20] >= 1 && c[20] < 65536 && c[21] >= 1 && c[21] < 65536) || !images[i])
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_layers: camera %u has no image or a size outside 1..65535", i);
    }
    *n_corr = 0;
    const size_t px = (size_t)cols * (size_t)rows;
    if (px == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip_ol::lab_tables tables;
    ochip_ol::lab_tables_build(&tables);
    const size_t Lpx = (size_t)L * px;
    const uint32_t nb = (uint32_t)((px + CHUNK - 1) / CHUNK);
    constexpr auto ENQ = ochip::copy_mode::enqueue;
    ochip::dev_scratch mem{ctx, "ochip_ortho_layers"};
    double *d_cams = nullptr;
    uint64_t *d_ids = nullptr, *d_images = nullptr, *d_bsum = nullptr, *d_id = nullptr;
    uint32_t *d_models = nullptr, *d_cam = nullptr, *d_knn = nullptr;
    ochip_ol::lab_tables *d_lab = nullptr;
    uint8_t *d_nvalid = nullptr, *d_bgra = nullptr, *d_counts = nullptr;
    float *d_fields = nullptr, *d_weight = nullptr;
    ochip_ol::corr_record *d_corr = nullptr;
    OCHIP_TRY(mem.upload(&d_cams, cams, (size_t)n_cams * ochip_ol::CAM_DOUBLES, ENQ));
    OCHIP_TRY(mem.upload(&d_ids, node_ids, n_cams, ENQ));
    OCHIP_TRY(mem.upload(&d_models, model_ids, n_cams, ENQ));
    OCHIP_TRY(mem.upload(&d_images, images, n_cams, ENQ));
    OCHIP_TRY(mem.upload<ochip_ol::lab_tables>(&d_lab, &tables, 1, ENQ));
    OCHIP_TRY(mem.alloc<uint8_t>(&d_nvalid, px));
    OCHIP_TRY(mem.alloc<uint32_t>(&d_cam, Lpx));
    OCHIP_TRY(mem.alloc<float>(&d_fields, Lpx * 4));
    OCHIP_TRY(mem.alloc<uint8_t>(&d_counts, px));
    OCHIP_TRY(mem.alloc<uint64_t>(&d_bsum, (size_t)nb + 1));
    if (!out_on_device)
    {
        OCHIP_TRY(mem.alloc<uint8_t>(&d_bgra, Lpx * 4));
        OCHIP_TRY(mem.alloc<uint64_t>(&d_id, Lpx));
        if (weight_out)
            OCHIP_TRY(mem.alloc<float>(&d_weight, Lpx));
    }
    if (knn_out)
        OCHIP_TRY(mem.alloc<uint32_t>(&d_knn, px * KNN));
    if (corr_capacity)
        OCHIP_TRY(mem.alloc<ochip_ol::corr_record>(&d_corr, (size_t)corr_capacity));
    const ochip_ol::band_planes B{L,
                                  cols,
                                  rows,
                                  d_nvalid,
                                  d_cam,
                                  out_on_device ? bgra_out : d_bgra,
                                  out_on_device ? id_out : d_id,
                                  out_on_device ? weight_out : d_weight,
                                  d_fields};
    const raster_args R = make_raster(raster4, cols, row0, rows);
    const uint64_t tiles = (uint64_t)R.tiles_x * (uint64_t)((rows + TILE - 1) / TILE);
    if (tiles >= ((uint64_t)1 << 31))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_layers: band too large");
    hipLaunchKernelGGL(ortho_layers_pass1, dim3((uint32_t)tiles), dim3(THREADS), 0, ctx->stream, m->args(), R, d_cams, n_cams,
                       (const uint8_t *const *)d_images, d_ids, d_lab, B, d_knn);
    hipLaunchKernelGGL(ortho_layers_count, dim3((uint32_t)((px + THREADS - 1) / THREADS)), dim3(THREADS), 0, ctx->stream, B, K,
                       d_counts);
    hipLaunchKernelGGL(ortho_layers_block_sums, dim3(nb), dim3(THREADS), 0, ctx->stream, d_counts, (int64_t)px, d_bsum);
    hipLaunchKernelGGL(ortho_layers_scan_top, dim3(1), dim3(THREADS), 0, ctx->stream, d_bsum, nb, d_bsum + nb);
    hipLaunchKernelGGL(ortho_layers_write, dim3(nb), dim3(THREADS), 0, ctx->stream, d_lab, B, K, d_models, d_counts, d_bsum, d_corr,
                       corr_capacity);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "ortho_layers kernel launch failed");
    const char *what = "ortho layers";
    uint64_t total = 0;
    OCHIP_TRY(copy_back(ctx, &total, d_bsum + nb, 8, what));
    if (!out_on_device)
    {
        OCHIP_TRY(copy_back(ctx, bgra_out, d_bgra, Lpx * 4, what));
        OCHIP_TRY(copy_back(ctx, id_out, d_id, Lpx * 8, what));
        OCHIP_TRY(copy_back(ctx, weight_out, d_weight, Lpx * 4, what));
    }
    OCHIP_TRY(copy_back(ctx, knn_out, d_knn, px * KNN * 4, what));
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ortho layers)");
    *n_corr = total;
    OCHIP_TRY(copy_back(ctx, corr_out, d_corr, (size_t)std::min<uint64_t>(total, corr_capacity) * sizeof(ochip_ol::corr_record), what));
    // the scratch goes back to the pool only once nothing can still write it
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ortho layers)");
    mem.release();
    return OCHIP_OK;
}

int ochip_ortho_band_cameras(ochip_ctx *ctx, const double *raster4, int32_t cols, int64_t rows, int64_t band_rows,
                             uint32_t n_cams, const double *cams, uint8_t *used_out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!raster4 || cols < 0 || rows < 0 || band_rows < 1 || (n_cams && !cams))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_band_cameras: bad argument");
    const uint64_t n_bands = (uint64_t)((rows + band_rows - 1) / band_rows);
    const size_t bytes = (size_t)n_bands * n_cams;
    if (bytes == 0)
        return OCHIP_OK;
    if (!used_out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_band_cameras: bad argument");
    if (cols == 0)
    {
        std::fill(used_out, used_out + bytes, (uint8_t)0);
        return OCHIP_OK;
    }
    const raster_args R = make_raster(raster4, cols, 0, rows);
    const uint64_t tiles_per_band_y = (uint64_t)((std::min(band_rows, rows) + TILE - 1) / TILE);
    if (n_bands * tiles_per_band_y > 65535 || R.tiles_x >= (1u << 31))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_band_cameras: more than 65535 tile rows in all bands");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_scratch mem{ctx, "ochip_ortho_band_cameras"};
    double *d_cams = nullptr;
    uint8_t *d_used = nullptr;
    OCHIP_TRY(mem.upload(&d_cams, cams, (size_t)n_cams * ochip_ol::CAM_DOUBLES, ochip::copy_mode::enqueue));
    OCHIP_TRY(mem.alloc<uint8_t>(&d_used, bytes));
    OCHIP_HIP(ctx, hipMemsetAsync(d_used, 0, bytes, ctx->stream));
    hipLaunchKernelGGL(ortho_band_cameras_kernel, dim3(R.tiles_x, (uint32_t)(n_bands * tiles_per_band_y)), dim3(THREADS), 0,
                       ctx->stream, R, band_rows, (uint32_t)tiles_per_band_y, d_cams, n_cams, d_used);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "ortho_band_cameras kernel launch failed");
    OCHIP_TRY(copy_back(ctx, used_out, d_used, bytes, "band cameras"));
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (band cameras)");
    mem.release();
    return OCHIP_OK;
}

// The image slots of a streamed render: one block of the context's pool, n_slots x slot_bytes, filled on the context's copy
// stream; marks are events on that stream which the compute stream can be made to wait for.
struct ochip_image_slots
{
    ochip_ctx *ctx = nullptr;
    ochip::dev_blocks mem;
    uint8_t *base = nullptr;
    uint32_t n_slots = 0;
    uint64_t slot_bytes = 0;
    std::vector<hipEvent_t> marks;
};

int ochip_image_slots_create(ochip_ctx *ctx, uint32_t n_slots, uint64_t slot_bytes, uint32_t n_marks, ochip_image_slots **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out || n_slots == 0 || slot_bytes == 0)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_image_slots_create: bad argument");
    *out = nullptr;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t copy;
    OCHIP_HIP(ctx, ochip_copy_stream(ctx, &copy));
    auto *s = new ochip_image_slots;
    s->ctx = ctx, s->mem.ctx = ctx, s->mem.what = "ochip_image_slots";
    s->n_slots = n_slots, s->slot_bytes = (slot_bytes + 255) / 256 * 256;
    s->base = (uint8_t *)s->mem.get((size_t)s->n_slots * s->slot_bytes);
    if (!s->base)
    {
        delete s;
        return OCHIP_ENOMEM;
    }
    for (uint32_t i = 0; i < n_marks; i++)
    {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess)
        {
            ochip_image_slots_destroy(s);
            return ochip_fail(ctx, OCHIP_EHIP, "ochip_image_slots_create: hipEventCreate failed");
        }
        s->marks.push_back(e);
    }
    *out = s;
    return OCHIP_OK;
}

void ochip_image_slots_destroy(ochip_image_slots *s)
{
    if (!s)
        return;
    // nothing may still write the block when it goes back to the pool
    if (s->ctx->copy_stream)
        (void)ochip_stream_wait(s->ctx, s->ctx->copy_stream);
    (void)ochip_stream_wait(s->ctx, s->ctx->stream);
    for (hipEvent_t e : s->marks)
        (void)hipEventDestroy(e);
    s->mem.release();
    delete s;
}

uint64_t ochip_image_slots_address(const ochip_image_slots *s, uint32_t slot)
{
    return s && slot < s->n_slots ? (uint64_t)(uintptr_t)(s->base + (size_t)slot * s->slot_bytes) : 0;
}

int ochip_image_slots_upload(ochip_image_slots *s, uint32_t slot, const void *host, uint64_t bytes)
{
    if (!s)
        return OCHIP_EINVAL;
    if (slot >= s->n_slots || !host || bytes > s->slot_bytes)
        return ochip_fail(s->ctx, OCHIP_EINVAL, "ochip_image_slots_upload: slot %u of %u, %llu bytes into %llu", slot, s->n_slots,
                          (unsigned long long)bytes, (unsigned long long)s->slot_bytes);
    OCHIP_HIP(s->ctx, hipSetDevice(s->ctx->device));
    OCHIP_HIP(s->ctx, hipMemcpyAsync(s->base + (size_t)slot * s->slot_bytes, host, (size_t)bytes, hipMemcpyHostToDevice,
                                     s->ctx->copy_stream));
    return OCHIP_OK;
}

int ochip_image_slots_mark(ochip_image_slots *s, uint32_t mark)
{
    if (!s)
        return OCHIP_EINVAL;
    if (mark >= s->marks.size())
        return ochip_fail(s->ctx, OCHIP_EINVAL, "ochip_image_slots_mark: mark %u of %zu", mark, s->marks.size());
    OCHIP_HIP(s->ctx, hipEventRecord(s->marks[mark], s->ctx->copy_stream));
    return OCHIP_OK;
}

int ochip_image_slots_wait(ochip_image_slots *s, uint32_t mark, int on_host)
{
    if (!s)
        return OCHIP_EINVAL;
    if (mark >= s->marks.size())
        return ochip_fail(s->ctx, OCHIP_EINVAL, "ochip_image_slots_wait: mark %u of %zu", mark, s->marks.size());
    if (on_host)
        OCHIP_HIP(s->ctx, hipEventSynchronize(s->marks[mark]));
    else
        OCHIP_HIP(s->ctx, hipStreamWaitEvent(s->ctx->stream, s->marks[mark], 0));
    return OCHIP_OK;
}

int ochip_image_slots_elapsed(ochip_image_slots *s, uint32_t from_mark, uint32_t to_mark, float *ms)
{
    if (!s)
        return OCHIP_EINVAL;
    if (from_mark >= s->marks.size() || to_mark >= s->marks.size() || !ms)
        return ochip_fail(s->ctx, OCHIP_EINVAL, "ochip_image_slots_elapsed: bad argument");
    OCHIP_HIP(s->ctx, hipEventSynchronize(s->marks[to_mark]));
    OCHIP_HIP(s->ctx, hipEventElapsedTime(ms, s->marks[from_mark], s->marks[to_mark]));
    return OCHIP_OK;
}
