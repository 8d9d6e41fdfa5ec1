// Points per triangle of a surface mesh on the device (the rule and the table: mesh_locate.hpp).
// The cloud is uploaded once per object; a count uploads the mesh's flat locate table and runs, on the context's stream:
//   locate_points     a thread a point: nearest centroid, walk; where[i], dist[i] and the sort key (class << shift | i) with
//                     class = the triangle, T for a point outside, T + 1 for one whose steps ran out
//   radix sort        rocPRIM, (key, dist) pairs: every triangle's distances become one segment in ascending point index; the
//                     keys are distinct, so the result is the one any correct sort gives
//   segment_sums      a wavefront a triangle: the segment's bounds by bisection of the sorted keys (count = its length, first
//                     = its first point), then sum += d, sum_sq += d * d in segment order - 64 distances loaded at once, one
//                     add chain fed lane by lane -, bit for bit the host's sequential loop
// No atomics anywhere: neither the counts nor the list of exhausted points (the tail of the sorted keys) need one, so a mesh
// of two triangles costs what one of ten thousand does, up to the two long add chains.
#include "ctx.hpp"
#include "live_handles.hpp"
#include "mesh_locate.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>
#include <memory>

namespace
{

using namespace ochip_ml;

constexpr int LOCATE_THREADS = 256, SUMS_THREADS = 256, WAVE = 64;

struct tri_result // what a count downloads per triangle
{
    uint32_t count, first;
    double sum, sum_sq;
};

__global__ __launch_bounds__(LOCATE_THREADS) void locate_points(const table t, const double *__restrict__ xyz, uint32_t n, int max_steps,
                                                                 unsigned shift, uint32_t *__restrict__ where, double *__restrict__ dist,
                                                                 unsigned long long *__restrict__ keys)
{
    const size_t i = (size_t)blockIdx.x * LOCATE_THREADS + threadIdx.x;
    if (i >= n)
        return;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const uint32_t w = walk(t, nearest_centroid(t, x, y), x, y, max_steps);
    uint32_t cls = t.T;
    double d = 0;
    if (w == NONE)
        ;
    else if (w & EXHAUSTED)
        cls = t.T + 1;
    else
    {
        cls = w;
        d = plane_distance(t, w, x, y, z);
    }
    where[i] = w;
    dist[i] = d;
    keys[i] = ((unsigned long long)cls << shift) | (unsigned long long)i;
}

// first index in keys[0, n) whose key is >= k
__device__ inline uint32_t lower_bound(const unsigned long long *keys, uint32_t n, unsigned long long k)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ inline double lane_value(double v, int lane) // v of lane `lane` (wave-uniform) in every lane
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// Wavefront w of the grid owns triangle w; wavefront T writes the start of the exhausted points' tail into *tail.
__global__ __launch_bounds__(SUMS_THREADS) void segment_sums(const unsigned long long *__restrict__ keys, const double *__restrict__ dist,
                                                              uint32_t n, uint32_t T, unsigned shift, tri_result *__restrict__ out,
                                                              uint32_t *__restrict__ tail)
{
    const uint32_t tri = blockIdx.x * (SUMS_THREADS / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (tri > T)
        return;
    if (tri == T)
    {
        if (lane == 0)
            *tail = lower_bound(keys, n, (unsigned long long)(T + 1) << shift);
        return;
    }
    // (every lane bisects the same keys: the bounds are wave-uniform without a broadcast)
    const uint64_t lo = lower_bound(keys, n, (unsigned long long)tri << shift), hi = lower_bound(keys, n, (unsigned long long)(tri + 1) << shift);
    double sum = 0, sum_sq = 0;
    double next = lo + lane < hi ? dist[lo + lane] : 0.0;
    for (uint64_t at = lo; at < hi; at += WAVE)
    {
        const double d = next, dd = d * d;
        if (at + WAVE < hi) // the load of the next 64 runs under this batch's add chain
            next = at + WAVE + lane < hi ? dist[at + WAVE + lane] : 0.0;
        const uint64_t left = hi - at;
        if (left >= WAVE)
        {
#pragma unroll
            for (int k = 0; k < WAVE; k++)
            {
                sum += lane_value(d, k);
                sum_sq += lane_value(dd, k);
            }
        }
        else
            for (int k = 0; k < (int)left; k++)
            {
                sum += lane_value(d, k);
                sum_sq += lane_value(dd, k);
            }
    }
    if (lane == 0)
    {
        tri_result r;
        r.count = (uint32_t)(hi - lo);
        r.first = hi > lo ? (uint32_t)(keys[lo] & ((1ull << shift) - 1)) : NONE;
        r.sum = sum, r.sum_sq = sum_sq;
        out[tri] = r;
    }
}

ochip::live_set<ochip_mesh_points> g_live; // the objects that exist

struct pinned // a page-locked block of the context's pool for the length of a call
{
    ochip_ctx *ctx;
    void *p = nullptr;
    explicit pinned(ochip_ctx *c) : ctx(c) {}
    ~pinned()
    {
        ochip_host_free(ctx, p);
    }
};

unsigned bits_for(uint64_t values) // bits that hold 0 .. values - 1, at least 1
{
    unsigned b = 1;
    while (b < 64 && (1ull << b) < values)
        b++;
    return b;
}

} // namespace

struct ochip_mesh_points
{
    ochip_ctx *ctx = nullptr;
    uint32_t n = 0;
    bool counted = false;    // where holds a count's result
    ochip::dev_blocks mem;   // everything below: sized by n alone, held until destroy
    double *xyz = nullptr;   // [n][3]
    uint32_t *where = nullptr;
    double *dist = nullptr, *dist_sorted = nullptr;
    unsigned long long *keys = nullptr, *keys_sorted = nullptr;
};

// The cloud of a live object for another entry of the library that reads it where it lies (xyz_export.hip): read-only, the
// object is not changed.  False for a handle that is not live.
bool ochip::mesh_points_view(const ochip_mesh_points *m, ochip_ctx **ctx, const double **xyz, uint32_t *n)
{
    if (!g_live.has(m))
        return false;
    *ctx = m->ctx, *xyz = m->xyz, *n = m->n;
    return true;
}

extern "C"
{

int ochip_mesh_points_create(ochip_ctx *ctx, const double *xyz, uint64_t n, ochip_mesh_points **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out || (n && !xyz))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_create: NULL argument");
    *out = nullptr;
    if (n >= (1ull << 32))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_create: %llu points, at most 2^32 - 1", (unsigned long long)n);
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<ochip_mesh_points> m(new ochip_mesh_points);
    m->ctx = ctx, m->n = (uint32_t)n;
    m->mem.ctx = ctx, m->mem.what = "ochip_mesh_points";
    if (n)
    {
        int rc = m->mem.alloc(&m->xyz, (size_t)n * 3);
        if (rc == OCHIP_OK)
            rc = m->mem.alloc(&m->where, (size_t)n);
        if (rc == OCHIP_OK)
            rc = m->mem.alloc(&m->dist, (size_t)n);
        if (rc == OCHIP_OK)
            rc = m->mem.alloc(&m->dist_sorted, (size_t)n);
        if (rc == OCHIP_OK)
            rc = m->mem.alloc(&m->keys, (size_t)n);
        if (rc == OCHIP_OK)
            rc = m->mem.alloc(&m->keys_sorted, (size_t)n);
        if (rc == OCHIP_OK)
        {
            // through a page-locked block: the copy runs at link speed and the caller's array is free on return
            pinned stage(ctx);
            rc = ochip_host_alloc(ctx, (size_t)n * 24, &stage.p);
            if (rc == OCHIP_OK)
            {
                std::memcpy(stage.p, xyz, (size_t)n * 24);
                hipError_t e = hipMemcpyAsync(m->xyz, stage.p, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess)
                    e = ochip_stream_wait(ctx, ctx->stream);
                if (e != hipSuccess)
                    rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_mesh_points_create: upload of %llu points failed: %s", (unsigned long long)n,
                                    hipGetErrorString(e));
            }
        }
        if (rc != OCHIP_OK)
        {
            m->mem.release(); // the one copy was waited for or never ran
            return rc;
        }
    }
    g_live.add(m.get());
    *out = m.release();
    return OCHIP_OK;
}

uint64_t ochip_mesh_points_size(const ochip_mesh_points *m)
{
    return g_live.has(m) ? m->n : 0;
}

int ochip_mesh_points_count(ochip_mesh_points *m, const ochip_locate_table *tab, int max_steps, uint32_t *count, uint32_t *first,
                            double *sum, double *sum_sq, uint32_t *exhausted, uint64_t exhausted_cap, uint64_t *n_exhausted)
{
    if (!g_live.has(m))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_mesh_points_count: not a live ochip_mesh_points object");
    ochip_ctx *ctx = m->ctx;
    if (!tab || !n_exhausted || max_steps < 0)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_count: bad argument (table %p, max_steps %d)", (const void *)tab, max_steps);
    table t;
    t.T = tab->n_triangles, t.vxy = tab->vertex_xy, t.nbr = tab->neighbours, t.plane = tab->plane, t.cx = tab->centroid_x;
    t.cy = tab->centroid_y, t.x0 = tab->x0, t.y0 = tab->y0, t.cell = tab->cell, t.nx = tab->nx, t.start = tab->start, t.items = tab->items;
    const std::string refusal = validate(t, tab->n_start, tab->n_items);
    if (!refusal.empty())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_count: inconsistent table: %s", refusal.c_str());
    const uint32_t T = t.T, n = m->n;
    if (T && (!count || !first || !sum || !sum_sq))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_count: an output array is NULL");
    *n_exhausted = 0;
    m->counted = false;
    for (uint32_t k = 0; k < T; k++)
        count[k] = 0, first[k] = NONE, sum[k] = 0, sum_sq[k] = 0;
    if (n == 0)
    {
        m->counted = true;
        return OCHIP_OK;
    }
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    if (T == 0) // no triangle: every point is outside
    {
        OCHIP_HIP(ctx, hipMemsetAsync(m->where, 0xFF, (size_t)n * 4, ctx->stream));
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
        m->counted = true;
        return OCHIP_OK;
    }
    const unsigned shift = bits_for(n), end_bit = shift + bits_for((uint64_t)T + 2);
    if (end_bit > 64)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_count: %u points x %u triangles exceed the 64-bit sort key", n, T);

    // the table in one page-locked block, one copy: doubles first (vxy 6T, plane 6T, cx T, cy T), then nbr 3T, start, items
    const size_t cells1 = tab->n_start, n_dbl = (size_t)T * 14, n_u32 = (size_t)T * 3 + cells1 + T;
    const size_t table_bytes = n_dbl * 8 + n_u32 * 4, result_bytes = (size_t)T * sizeof(tri_result) + 8;
    pinned stage(ctx);
    OCHIP_TRY(ochip_host_alloc(ctx, table_bytes > result_bytes ? table_bytes : result_bytes, &stage.p));
    {
        double *hd = static_cast<double *>(stage.p);
        std::memcpy(hd, t.vxy, (size_t)T * 48);
        std::memcpy(hd + (size_t)T * 6, t.plane, (size_t)T * 48);
        std::memcpy(hd + (size_t)T * 12, t.cx, (size_t)T * 8);
        std::memcpy(hd + (size_t)T * 13, t.cy, (size_t)T * 8);
        uint32_t *hu = reinterpret_cast<uint32_t *>(hd + n_dbl);
        std::memcpy(hu, t.nbr, (size_t)T * 12);
        std::memcpy(hu + (size_t)T * 3, t.start, cells1 * 4);
        std::memcpy(hu + (size_t)T * 3 + cells1, t.items, (size_t)T * 4);
    }
    ochip::dev_scratch scratch{ctx, "ochip_mesh_points_count"};
    void *tab_dev = nullptr;
    OCHIP_TRY(scratch.upload_bytes(&tab_dev, stage.p, table_bytes, ochip::copy_mode::enqueue));
    {
        const double *dd = static_cast<const double *>(tab_dev);
        t.vxy = dd, t.plane = dd + (size_t)T * 6, t.cx = dd + (size_t)T * 12, t.cy = dd + (size_t)T * 13;
        const uint32_t *du = reinterpret_cast<const uint32_t *>(dd + n_dbl);
        t.nbr = du, t.start = du + (size_t)T * 3, t.items = du + (size_t)T * 3 + cells1;
    }
    tri_result *res_dev = nullptr; // [T] results, then the tail's start
    OCHIP_TRY(scratch.upload_bytes(reinterpret_cast<void **>(&res_dev), nullptr, result_bytes, ochip::copy_mode::enqueue));
    uint32_t *tail_dev = reinterpret_cast<uint32_t *>(res_dev + T);
    size_t sort_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, m->keys, m->keys_sorted, m->dist, m->dist_sorted, (size_t)n, 0u, end_bit,
                                  (hipStream_t)ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_mesh_points_count: the sort's storage query failed");
    void *sort_tmp = scratch.get(sort_bytes);
    if (!sort_tmp)
        return OCHIP_ENOMEM;

    const uint32_t locate_blocks = (uint32_t)(((size_t)n + LOCATE_THREADS - 1) / LOCATE_THREADS);
    hipLaunchKernelGGL(locate_points, dim3(locate_blocks), dim3(LOCATE_THREADS), 0, ctx->stream, t, m->xyz, n, max_steps, shift, m->where,
                       m->dist, m->keys);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "locate_points launch failed");
    OCHIP_HIP(ctx, rocprim::radix_sort_pairs(sort_tmp, sort_bytes, m->keys, m->keys_sorted, m->dist, m->dist_sorted, (size_t)n, 0u, end_bit,
                                             (hipStream_t)ctx->stream));
    const uint32_t sums_blocks = (uint32_t)(((size_t)T + 1 + SUMS_THREADS / WAVE - 1) / (SUMS_THREADS / WAVE));
    hipLaunchKernelGGL(segment_sums, dim3(sums_blocks), dim3(SUMS_THREADS), 0, ctx->stream, m->keys_sorted, m->dist_sorted, n, T, shift,
                       res_dev, tail_dev);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "segment_sums launch failed");
    // (the table's copy has run before the results' copy writes the same page-locked block: one stream)
    OCHIP_HIP(ctx, hipMemcpyAsync(stage.p, res_dev, result_bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    const tri_result *res = static_cast<const tri_result *>(stage.p);
    for (uint32_t k = 0; k < T; k++)
        count[k] = res[k].count, first[k] = res[k].first, sum[k] = res[k].sum, sum_sq[k] = res[k].sum_sq;
    uint32_t tail = 0;
    std::memcpy(&tail, res + T, 4);
    m->counted = true;
    if (tail > n)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_mesh_points_count: the exhausted points start at %u of %u", tail, n);
    const uint64_t n_ex = n - tail;
    *n_exhausted = n_ex;
    if (n_ex)
    {
        if (!exhausted || exhausted_cap < n_ex)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_count: %llu points exhausted their steps, room for %llu",
                              (unsigned long long)n_ex, (unsigned long long)(exhausted ? exhausted_cap : 0));
        pinned back(ctx);
        OCHIP_TRY(ochip_host_alloc(ctx, (size_t)n_ex * 8, &back.p));
        OCHIP_HIP(ctx, hipMemcpyAsync(back.p, m->keys_sorted + tail, (size_t)n_ex * 8, hipMemcpyDeviceToHost, ctx->stream));
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
        const unsigned long long *k64 = static_cast<const unsigned long long *>(back.p);
        for (uint64_t k = 0; k < n_ex; k++)
            exhausted[k] = (uint32_t)(k64[k] & ((1ull << shift) - 1));
    }
    scratch.release();
    return OCHIP_OK;
}

int ochip_mesh_points_where(ochip_mesh_points *m, uint32_t *where)
{
    if (!g_live.has(m))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_mesh_points_where: not a live ochip_mesh_points object");
    ochip_ctx *ctx = m->ctx;
    if (!m->counted)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_mesh_points_where: no count has run on this object");
    if (m->n == 0)
        return OCHIP_OK;
    if (!where)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_mesh_points_where: the output array is NULL");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    OCHIP_HIP(ctx, hipMemcpyAsync(where, m->where, (size_t)m->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    return OCHIP_OK;
}

void ochip_mesh_points_destroy(ochip_mesh_points *m)
{
    if (!g_live.remove(m))
        return;
    if (!m->mem.empty() && m->ctx->stream.opened()) // nothing may still touch the blocks when they go back to the pool
        (void)ochip_stream_wait(m->ctx, m->ctx->stream);
    m->mem.release();
    delete m;
}

} // extern "C"
