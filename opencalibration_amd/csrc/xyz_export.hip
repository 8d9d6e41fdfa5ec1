// The point cloud file on the device (the rules: xyz_export.hpp).  An object holds one flat cloud.
// bounds, on the context's stream:
//   axis_keys         a thread a point: the three integer cells, a flag for a coordinate without one
//   radix sort + run-length encode (rocPRIM), per axis: the (key, count) rows in ascending key order, exact for any span;
//                     the few rows come back and the box is filterOutliers' walk on the host
// text_size:
//   format_lines      a thread a point: the box test, the three numbers straight into the point's 48-byte slot in LDS, the
//                     block's slots stored as one contiguous run; the line's length (0: dropped, 255: a number the integer
//                     formatter does not cover - the block is flagged and the host formats that line with snprintf)
//   exclusive scan    rocPRIM, 64-bit, over the lengths: every line's offset in the file, and the file's size
// text:
//   scatter_lines     a workgroup 256 points: their lines packed in LDS at the file's alignment, then written as whole
//                     16-byte words (bytes at the two ragged ends)
// Point order throughout, no atomics: the same bytes on every run.
#include "ctx.hpp"
#include "live_handles.hpp"
#include "xyz_export.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cstring>
#include <memory>
#include <vector>

namespace
{

using namespace ochip_xe;

constexpr int THREADS = 256;
constexpr int MAX_LINE = 42;                                            // 3 * 13 + 3
constexpr int SLOT_WORDS = SLOT / 16;                                   // uint4 per slot
constexpr int STAGE_WORDS = (THREADS * MAX_LINE + 15 + 15) / 16;        // the packed lines of a block after <= 15 bytes of lead
constexpr uint8_t LEN_FALLBACK = 255;

__global__ __launch_bounds__(THREADS) void axis_keys(const double *__restrict__ xyz, uint32_t n, long long *__restrict__ keys,
                                                     uint32_t *__restrict__ undefined)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n)
        return;
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
        const double v = xyz[3 * i + a];
        const bool ok = key_defined(v);
        bad |= !ok;
        keys[(size_t)a * n + i] = ok ? axis_key(v) : 0;
    }
    if (bad)
        *undefined = 1; // every writer stores the same value
}

// One number at the end of the line that stands in LDS; false when the formatter does not cover it
__device__ inline bool append_number(double v, char *line, int &at)
{
    const int l = format_g6(v, line + at);
    at += l;
    return l != 0;
}

__global__ __launch_bounds__(THREADS) void format_lines(const double *__restrict__ xyz, uint32_t n, const bounds3 box, uint4 *__restrict__ slots,
                                                        uint8_t *__restrict__ len, uint8_t *__restrict__ block_flag)
{
    __shared__ uint4 lines[THREADS * SLOT_WORDS];
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    char *line = reinterpret_cast<char *>(lines) + threadIdx.x * SLOT;
    int fallback = 0;
    if (i < n)
    {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        int l = 0;
        if (inbounds(box, x, y, z))
        {
            bool mine = append_number(x, line, l);
            line[l++] = ',';
            mine &= append_number(y, line, l);
            line[l++] = ',';
            mine &= append_number(z, line, l);
            line[l++] = '\n';
            if (!mine)
                l = LEN_FALLBACK, fallback = 1;
        }
        len[i] = (uint8_t)l;
    }
    fallback = __syncthreads_or(fallback);
    if (threadIdx.x == 0)
        block_flag[blockIdx.x] = (uint8_t)fallback;
    // (slots is a whole number of blocks long)
    uint4 *dst = slots + (size_t)blockIdx.x * (THREADS * SLOT_WORDS);
#pragma unroll
    for (int k = 0; k < SLOT_WORDS; k++)
        dst[k * THREADS + threadIdx.x] = lines[k * THREADS + threadIdx.x];
}

struct line_bytes // a length as the scan adds it: a line that is not there yet counts nothing
{
    __host__ __device__ unsigned long long operator()(uint8_t l) const
    {
        return l > MAX_LINE ? 0ull : (unsigned long long)l;
    }
};
struct line_kept
{
    __host__ __device__ unsigned long long operator()(uint8_t l) const
    {
        return l != 0 ? 1ull : 0ull;
    }
};

// offsets [n + 1] (the last: the file's size); out: the file, a device block whose address is 16-byte aligned
__global__ __launch_bounds__(THREADS) void scatter_lines(const uint4 *__restrict__ slots, const uint8_t *__restrict__ len,
                                                         const unsigned long long *__restrict__ offsets, uint32_t n, char *__restrict__ out)
{
    __shared__ uint4 lines[THREADS * SLOT_WORDS];
    __shared__ uint4 stage[STAGE_WORDS];
    const size_t first = (size_t)blockIdx.x * THREADS, i = first + threadIdx.x;
    const size_t last = first + THREADS < n ? first + THREADS : n;
    const unsigned long long base = offsets[first], total = offsets[last] - base; // total <= THREADS * MAX_LINE
    const uint32_t lead = (uint32_t)(base & 15u);
    const uint4 *src = slots + (size_t)blockIdx.x * (THREADS * SLOT_WORDS);
#pragma unroll
    for (int k = 0; k < SLOT_WORDS; k++)
        lines[k * THREADS + threadIdx.x] = src[k * THREADS + threadIdx.x];
    __syncthreads();
    if (i < n)
    {
        uint32_t l = len[i];
        l = l > MAX_LINE ? 0 : l;
        const uint32_t at = (uint32_t)(offsets[i] - base) + lead;
        const char *line = reinterpret_cast<const char *>(lines) + threadIdx.x * SLOT;
        char *to = reinterpret_cast<char *>(stage);
        if (at + l <= STAGE_WORDS * 16)
            for (uint32_t k = 0; k < l; k++)
                to[at + k] = line[k];
    }
    __syncthreads();
    // word w of the stage is file bytes [base - lead + 16 w, + 16): whole words as one store, the ends byte by byte
    const uint32_t begin = lead, end = lead + (uint32_t)total, words = (end + 15) / 16;
    char *aligned = out + (base - lead);
    for (uint32_t w = threadIdx.x; w < words && w < STAGE_WORDS; w += THREADS)
    {
        const uint32_t b0 = w * 16, b1 = b0 + 16;
        if (b0 >= begin && b1 <= end)
            reinterpret_cast<uint4 *>(aligned)[w] = stage[w];
        else
        {
            const char *from = reinterpret_cast<const char *>(stage);
            for (uint32_t b = b0 < begin ? begin : b0; b < b1 && b < end; b++)
                aligned[b] = from[b];
        }
    }
}

__global__ __launch_bounds__(THREADS) void format_numbers(const double *__restrict__ v, size_t n, uint4 *__restrict__ text, uint8_t *__restrict__ len)
{
    __shared__ uint4 cells[THREADS];
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n)
        return;
    cells[threadIdx.x] = make_uint4(0, 0, 0, 0);
    len[i] = (uint8_t)format_g6(v[i], reinterpret_cast<char *>(&cells[threadIdx.x]));
    text[i] = cells[threadIdx.x];
}

ochip::live_set<ochip_xyz_export> g_live; // the objects that exist

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

size_t blocks_of(uint64_t n)
{
    return (size_t)((n + THREADS - 1) / THREADS);
}

// "%g" of one number by the integer formatter, else by the C library: what the host does for a line the device left
int format_any(double v, char *out)
{
    const int l = format_g6(v, out);
    return l ? l : std::snprintf(out, NUMBER_CHARS, "%g", v);
}

} // namespace

struct ochip_xyz_export
{
    ochip_ctx *ctx = nullptr;
    uint32_t n = 0;
    ochip::dev_blocks mem; // everything below, held until destroy
    double *xyz = nullptr; // [n][3]
    // what text_size leaves for text
    uint4 *slots = nullptr;              // [blocks][THREADS] slots
    uint8_t *len = nullptr;              // [n + 1], the last 0
    uint8_t *block_flag = nullptr;       // [blocks]
    unsigned long long *offsets = nullptr; // [n + 1]
    unsigned long long *kept_dev = nullptr;
    bool sized = false;
    uint64_t bytes = 0, kept = 0;
};

namespace
{
int new_export(ochip_ctx *ctx, uint64_t n, const char *who, std::unique_ptr<ochip_xyz_export> &e)
{
    if (n >= (1ull << 32))
        return ochip_fail(ctx, OCHIP_EINVAL, "%s: %llu points, at most 2^32 - 1", who, (unsigned long long)n);
    hipError_t err = hipSetDevice(ctx->device);
    if (err != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "%s: hipSetDevice failed: %s", who, hipGetErrorString(err));
    e.reset(new ochip_xyz_export);
    e->ctx = ctx, e->n = (uint32_t)n;
    e->mem.ctx = ctx, e->mem.what = "ochip_xyz_export";
    return n ? e->mem.alloc(&e->xyz, (size_t)n * 3) : OCHIP_OK;
}

int publish(std::unique_ptr<ochip_xyz_export> &e, ochip_xyz_export **out)
{
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

// The lines of the flagged blocks that the device left to the host: formatted here, their text and lengths uploaded
int format_left_lines(ochip_xyz_export *e, const uint8_t *flags, size_t blocks)
{
    ochip_ctx *ctx = e->ctx;
    std::vector<double> xyz(THREADS * 3);
    std::vector<uint8_t> len(THREADS);
    for (size_t b = 0; b < blocks; b++)
    {
        if (!flags[b])
            continue;
        const size_t first = b * THREADS, count = e->n - first < THREADS ? e->n - first : THREADS;
        OCHIP_HIP(ctx, hipMemcpy(xyz.data(), e->xyz + first * 3, count * 24, hipMemcpyDeviceToHost));
        OCHIP_HIP(ctx, hipMemcpy(len.data(), e->len + first, count, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < count; k++)
        {
            if (len[k] != LEN_FALLBACK)
                continue;
            char num[3][NUMBER_CHARS], line[SLOT] = {0};
            int l[3];
            for (int a = 0; a < 3; a++)
            {
                l[a] = format_any(xyz[3 * k + a], num[a]);
                if (l[a] <= 0 || l[a] > 13)
                    return ochip_fail(ctx, OCHIP_EHIP, "ochip_xyz_export: a number of %d characters", l[a]);
            }
            const uint8_t total = (uint8_t)join_line(num[0], l[0], num[1], l[1], num[2], l[2], line);
            // (a workgroup stores its slots as they lie in LDS, point after point: point i's slot is at byte i * SLOT)
            char *slot = reinterpret_cast<char *>(e->slots) + (first + k) * SLOT;
            OCHIP_HIP(ctx, hipMemcpy(slot, line, SLOT, hipMemcpyHostToDevice));
            OCHIP_HIP(ctx, hipMemcpy(e->len + first + k, &total, 1, hipMemcpyHostToDevice));
        }
    }
    return OCHIP_OK;
}

// offsets and the kept count from the lengths, enqueued
int scan_lengths(ochip_xyz_export *e, ochip::dev_scratch &scratch)
{
    ochip_ctx *ctx = e->ctx;
    const size_t n1 = (size_t)e->n + 1;
    auto as_bytes = rocprim::make_transform_iterator(e->len, line_bytes());
    auto as_kept = rocprim::make_transform_iterator(e->len, line_kept());
    size_t scan_bytes = 0, reduce_bytes = 0;
    OCHIP_HIP(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, as_bytes, e->offsets, 0ull, n1, rocprim::plus<unsigned long long>(),
                                           (hipStream_t)ctx->stream));
    OCHIP_HIP(ctx, rocprim::reduce(nullptr, reduce_bytes, as_kept, e->kept_dev, 0ull, n1, rocprim::plus<unsigned long long>(),
                                   (hipStream_t)ctx->stream));
    void *scan_tmp = scratch.get(scan_bytes), *reduce_tmp = scratch.get(reduce_bytes);
    if (!scan_tmp || !reduce_tmp)
        return OCHIP_ENOMEM;
    OCHIP_HIP(ctx, rocprim::exclusive_scan(scan_tmp, scan_bytes, as_bytes, e->offsets, 0ull, n1, rocprim::plus<unsigned long long>(),
                                           (hipStream_t)ctx->stream));
    OCHIP_HIP(ctx, rocprim::reduce(reduce_tmp, reduce_bytes, as_kept, e->kept_dev, 0ull, n1, rocprim::plus<unsigned long long>(),
                                   (hipStream_t)ctx->stream));
    return OCHIP_OK;
}
} // namespace

extern "C"
{

int ochip_xyz_export_create(ochip_ctx *ctx, const double *xyz, uint64_t n, ochip_xyz_export **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out || (n && !xyz))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_create: NULL argument");
    *out = nullptr;
    std::unique_ptr<ochip_xyz_export> e;
    OCHIP_TRY(new_export(ctx, n, "ochip_xyz_export_create", e));
    if (n)
    {
        // through a page-locked block: the copy runs at link speed and the caller's array is free on return
        pinned stage(ctx);
        int rc = ochip_host_alloc(ctx, (size_t)n * 24, &stage.p);
        if (rc == OCHIP_OK)
        {
            std::memcpy(stage.p, xyz, (size_t)n * 24);
            hipError_t err = hipMemcpyAsync(e->xyz, stage.p, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream);
            if (err == hipSuccess)
                err = ochip_stream_wait(ctx, ctx->stream);
            if (err != hipSuccess)
                rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_xyz_export_create: upload of %llu points failed: %s", (unsigned long long)n,
                                hipGetErrorString(err));
        }
        if (rc != OCHIP_OK)
        {
            e->mem.release(); // the one copy was waited for or never ran
            return rc;
        }
    }
    return publish(e, out);
}

int ochip_xyz_export_create_from_points(ochip_ctx *ctx, const ochip_mesh_points *const *clouds, uint64_t n_clouds, ochip_xyz_export **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out || (n_clouds && !clouds))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_create_from_points: NULL argument");
    *out = nullptr;
    uint64_t n = 0;
    std::vector<std::pair<const double *, uint32_t>> parts;
    for (uint64_t c = 0; c < n_clouds; c++)
    {
        ochip_ctx *owner = nullptr;
        const double *xyz = nullptr;
        uint32_t count = 0;
        if (!ochip::mesh_points_view(clouds[c], &owner, &xyz, &count))
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_create_from_points: cloud %llu is not a live ochip_mesh_points object",
                              (unsigned long long)c);
        if (owner != ctx)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_create_from_points: cloud %llu belongs to another context",
                              (unsigned long long)c);
        parts.emplace_back(xyz, count);
        n += count;
    }
    std::unique_ptr<ochip_xyz_export> e;
    OCHIP_TRY(new_export(ctx, n, "ochip_xyz_export_create_from_points", e));
    size_t at = 0;
    hipError_t err = hipSuccess;
    for (const auto &p : parts)
    {
        if (p.second && err == hipSuccess)
            err = hipMemcpyAsync(e->xyz + at * 3, p.first, (size_t)p.second * 24, hipMemcpyDeviceToDevice, ctx->stream);
        at += p.second;
    }
    if (n && err == hipSuccess)
        err = ochip_stream_wait(ctx, ctx->stream);
    if (err != hipSuccess)
    {
        if (ctx->stream.opened())
            (void)ochip_stream_wait(ctx, ctx->stream);
        e->mem.release();
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_xyz_export_create_from_points: device copy failed: %s", hipGetErrorString(err));
    }
    return publish(e, out);
}

uint64_t ochip_xyz_export_size(const ochip_xyz_export *e)
{
    return g_live.has(e) ? e->n : 0;
}

int ochip_xyz_export_bounds(ochip_xyz_export *e, int64_t *bounds6)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_xyz_export_bounds: not a live ochip_xyz_export object");
    ochip_ctx *ctx = e->ctx;
    if (!bounds6)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_bounds: the output array is NULL");
    for (int k = 0; k < 6; k++)
        bounds6[k] = 0;
    const size_t n = e->n;
    if (n == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_scratch scratch{ctx, "ochip_xyz_export_bounds"};
    long long *keys = nullptr, *sorted = nullptr, *unique = nullptr;
    uint32_t *counts = nullptr, *small = nullptr; // small: the runs of the three axes, then the flag
    OCHIP_TRY(scratch.alloc(&keys, 3 * n));
    OCHIP_TRY(scratch.alloc(&sorted, 3 * n));
    OCHIP_TRY(scratch.alloc(&unique, 3 * n));
    OCHIP_TRY(scratch.alloc(&counts, 3 * n));
    OCHIP_TRY(scratch.alloc(&small, 4));
    size_t sort_bytes = 0, rle_bytes = 0;
    OCHIP_HIP(ctx, rocprim::radix_sort_keys(nullptr, sort_bytes, keys, sorted, n, 0u, 64u, (hipStream_t)ctx->stream));
    OCHIP_HIP(ctx, rocprim::run_length_encode(nullptr, rle_bytes, sorted, (unsigned int)n, unique, counts, small, (hipStream_t)ctx->stream));
    void *sort_tmp = scratch.get(sort_bytes), *rle_tmp = scratch.get(rle_bytes);
    if (!sort_tmp || !rle_tmp)
        return OCHIP_ENOMEM;
    OCHIP_HIP(ctx, hipMemsetAsync(small, 0, 16, ctx->stream));
    hipLaunchKernelGGL(axis_keys, dim3((uint32_t)blocks_of(n)), dim3(THREADS), 0, ctx->stream, e->xyz, (uint32_t)n, keys, small + 3);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "axis_keys launch failed");
    for (int a = 0; a < 3; a++)
    {
        OCHIP_HIP(ctx, rocprim::radix_sort_keys(sort_tmp, sort_bytes, keys + a * n, sorted + a * n, n, 0u, 64u, (hipStream_t)ctx->stream));
        OCHIP_HIP(ctx, rocprim::run_length_encode(rle_tmp, rle_bytes, sorted + a * n, (unsigned int)n, unique + a * n, counts + a * n,
                                                  small + a, (hipStream_t)ctx->stream));
    }
    uint32_t head[4] = {0, 0, 0, 0};
    OCHIP_HIP(ctx, hipMemcpyAsync(head, small, 16, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    if (head[3])
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_bounds: a coordinate is not finite or not below 2^63 in magnitude");
    size_t rows_total = 0;
    for (int a = 0; a < 3; a++)
    {
        if (head[a] == 0 || head[a] > n)
            return ochip_fail(ctx, OCHIP_EHIP, "ochip_xyz_export_bounds: axis %d has %u rows for %zu points", a, head[a], n);
        rows_total += head[a];
    }
    pinned back(ctx);
    OCHIP_TRY(ochip_host_alloc(ctx, rows_total * 12, &back.p));
    long long *hk = static_cast<long long *>(back.p);
    uint32_t *hc = reinterpret_cast<uint32_t *>(hk + rows_total);
    size_t at = 0;
    for (int a = 0; a < 3; a++)
    {
        OCHIP_HIP(ctx, hipMemcpyAsync(hk + at, unique + a * n, (size_t)head[a] * 8, hipMemcpyDeviceToHost, ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(hc + at, counts + a * n, (size_t)head[a] * 4, hipMemcpyDeviceToHost, ctx->stream));
        at += head[a];
    }
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    scratch.release();
    at = 0;
    for (int a = 0; a < 3; a++)
    {
        std::vector<int64_t> k(head[a]);
        std::vector<uint64_t> c(head[a]);
        for (uint32_t r = 0; r < head[a]; r++)
            k[r] = hk[at + r], c[r] = hc[at + r];
        const std::pair<int64_t, int64_t> box = dimbox(k.data(), c.data(), k.size(), n);
        bounds6[2 * a] = box.first, bounds6[2 * a + 1] = box.second;
        at += head[a];
    }
    return OCHIP_OK;
}

int ochip_xyz_export_text_size(ochip_xyz_export *e, const int64_t *bounds6, uint64_t *bytes, uint64_t *kept)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_xyz_export_text_size: not a live ochip_xyz_export object");
    ochip_ctx *ctx = e->ctx;
    if (!bytes || !kept)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_text_size: an output pointer is NULL");
    *bytes = 0, *kept = 0;
    e->sized = false;
    const size_t n = e->n, blocks = blocks_of(n);
    if (n == 0)
    {
        e->bytes = 0, e->kept = 0, e->sized = true;
        return OCHIP_OK;
    }
    bounds3 box = {{0, 0, 0}, {0, 0, 0}}; // the box toXYZ takes for "no filter"
    if (bounds6)
        for (int a = 0; a < 3; a++)
            box.lo[a] = bounds6[2 * a], box.hi[a] = bounds6[2 * a + 1];
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    if (!e->slots)
    {
        int rc = e->mem.alloc(&e->slots, blocks * THREADS * SLOT_WORDS);
        if (rc == OCHIP_OK)
            rc = e->mem.alloc(&e->len, n + 1);
        if (rc == OCHIP_OK)
            rc = e->mem.alloc(&e->block_flag, blocks);
        if (rc == OCHIP_OK)
            rc = e->mem.alloc(&e->offsets, n + 1);
        if (rc == OCHIP_OK)
            rc = e->mem.alloc(&e->kept_dev, 1);
        if (rc != OCHIP_OK)
        {
            e->slots = nullptr; // (the blocks taken so far stay with the object until destroy)
            return rc;
        }
    }
    ochip::dev_scratch scratch{ctx, "ochip_xyz_export_text_size"};
    pinned back(ctx);
    OCHIP_TRY(ochip_host_alloc(ctx, blocks + 16, &back.p));
    uint8_t *flags = static_cast<uint8_t *>(back.p) + 16;
    unsigned long long *totals = static_cast<unsigned long long *>(back.p); // the file's size, the lines kept
    OCHIP_HIP(ctx, hipMemsetAsync(e->len + n, 0, 1, ctx->stream));
    hipLaunchKernelGGL(format_lines, dim3((uint32_t)blocks), dim3(THREADS), 0, ctx->stream, e->xyz, (uint32_t)n, box, e->slots, e->len,
                       e->block_flag);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "format_lines launch failed");
    // the scan runs at once: a cloud with a line left to the host (flags) is rare and pays a second scan
    for (int pass = 0; pass < 2; pass++)
    {
        OCHIP_TRY(scan_lengths(e, scratch));
        OCHIP_HIP(ctx, hipMemcpyAsync(totals, e->offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(totals + 1, e->kept_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
        if (pass == 0)
            OCHIP_HIP(ctx, hipMemcpyAsync(flags, e->block_flag, blocks, hipMemcpyDeviceToHost, ctx->stream));
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
        bool left = false;
        for (size_t b = 0; pass == 0 && b < blocks; b++)
            left = left || flags[b];
        if (!left)
            break;
        OCHIP_TRY(format_left_lines(e, flags, blocks));
    }
    scratch.release();
    if (totals[0] > (unsigned long long)n * MAX_LINE || totals[1] > n)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_xyz_export_text_size: %llu bytes in %llu lines of %zu points", totals[0], totals[1], n);
    e->bytes = totals[0], e->kept = totals[1], e->sized = true;
    *bytes = e->bytes, *kept = e->kept;
    return OCHIP_OK;
}

int ochip_xyz_export_text(ochip_xyz_export *e, char *out, uint64_t cap)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_xyz_export_text: not a live ochip_xyz_export object");
    ochip_ctx *ctx = e->ctx;
    if (!e->sized)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_xyz_export_text: ochip_xyz_export_text_size has not run on this object");
    if (cap < e->bytes)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_text: room for %llu bytes, the text has %llu", (unsigned long long)cap,
                          (unsigned long long)e->bytes);
    if (e->bytes == 0)
        return OCHIP_OK;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_xyz_export_text: the output array is NULL");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_scratch scratch{ctx, "ochip_xyz_export_text"};
    char *file = nullptr;
    OCHIP_TRY(scratch.alloc(&file, (size_t)e->bytes + 16));
    pinned back(ctx);
    OCHIP_TRY(ochip_host_alloc(ctx, (size_t)e->bytes, &back.p));
    hipLaunchKernelGGL(scatter_lines, dim3((uint32_t)blocks_of(e->n)), dim3(THREADS), 0, ctx->stream, e->slots, e->len, e->offsets, e->n, file);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "scatter_lines launch failed");
    OCHIP_HIP(ctx, hipMemcpyAsync(back.p, file, (size_t)e->bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    scratch.release();
    std::memcpy(out, back.p, (size_t)e->bytes);
    return OCHIP_OK;
}

void ochip_xyz_export_destroy(ochip_xyz_export *e)
{
    if (!g_live.remove(e))
        return;
    if (!e->mem.empty() && e->ctx->stream.opened()) // nothing may still touch the blocks when they go back to the pool
        (void)ochip_stream_wait(e->ctx, e->ctx->stream);
    e->mem.release();
    delete e;
}

int ochip_debug_format_g6(ochip_ctx *ctx, const double *values, uint64_t n, char *text16, uint8_t *len)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (n && (!values || !text16 || !len))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_format_g6: NULL argument");
    if (n == 0)
        return OCHIP_OK;
    if (n >= (1ull << 32))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_format_g6: %llu values, at most 2^32 - 1", (unsigned long long)n);
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_scratch scratch{ctx, "ochip_debug_format_g6"};
    double *v = nullptr;
    uint4 *text = nullptr;
    uint8_t *l = nullptr;
    OCHIP_TRY(scratch.upload(&v, values, (size_t)n, ochip::copy_mode::blocking));
    OCHIP_TRY(scratch.alloc(&text, (size_t)n));
    OCHIP_TRY(scratch.alloc(&l, (size_t)n));
    hipLaunchKernelGGL(format_numbers, dim3((uint32_t)blocks_of(n)), dim3(THREADS), 0, ctx->stream, v, (size_t)n, text, l);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "format_numbers launch failed");
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    OCHIP_HIP(ctx, hipMemcpy(text16, text, (size_t)n * 16, hipMemcpyDeviceToHost));
    OCHIP_HIP(ctx, hipMemcpy(len, l, (size_t)n, hipMemcpyDeviceToHost));
    scratch.release();
    return OCHIP_OK;
}

} // extern "C"
