// Averaged overview levels of the orthomosaic and the DSM on the device (the rule and the builder's
// bookkeeping: ortho_overview.hpp).  Two kernels, both for 4-byte pixels under either rule:
//   overview_fused  a workgroup of 256 threads owns an aligned 64 x 64 block of level 0, reads it once - a thread its 4 x 4
//                   patch, four 16-byte loads - and writes the block's pixels of every level down to 6: levels 1 and 2 from
//                   the thread's registers, levels 3 to 6 through two 1 KB planes of LDS.  The cascade of an aligned block
//                   reads that block alone, so the result is the plain route's bit for bit.
//   overview_plain  one level from the one before, a thread a pixel: the levels above 6, the rows of a band outside whole
//                   aligned blocks, and everything under the test hook overview_per_level.
// Plain launches on the context's stream; no host wait when the band and the levels are on the device.
#include "ctx.hpp"
#include "ortho_overview.hpp"

#include <memory>
#include <vector>

namespace
{

using namespace ochip_ov;

constexpr int FUSED_THREADS = 256, PLAIN_THREADS = 256;
static_assert(FUSED_DEPTH == 6 && FUSED_BLOCK == 64, "overview_fused is written for 64 x 64 blocks");

template <class T> struct fused_args
{
    const T *src;     // the band: level-0 rows from src_row0 on
    int64_t src_row0; // (a multiple of 64 rows below row_a or equal to it)
    int64_t row_a;    // first level-0 row of block row 0, a multiple of 64
    int64_t w, h;     // level 0's whole size
    int depth;        // levels written, 1 .. 6
    int vec;          // rows of level 0 are 16-byte aligned: w % 4 == 0 and an aligned base
    T *dst[FUSED_DEPTH + 1]; // whole levels, [1 .. depth]
};

template <class R> __global__ __launch_bounds__(FUSED_THREADS) void overview_fused(const fused_args<typename R::type> A)
{
    using T = typename R::type;
    __shared__ T plane[2][256];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t x0 = (int64_t)blockIdx.x * 64 + tx * 4, y0 = A.row_a + (int64_t)blockIdx.y * 64 + ty * 4;

    // level 0: the thread's 4 x 4 patch; pixels that do not exist stay 0 and are never counted
    T v[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
            v[i][j] = T(0);
        const int64_t y = y0 + i;
        if (y < A.h && x0 < A.w)
        {
            const T *row = A.src + (size_t)(y - A.src_row0) * (size_t)A.w + (size_t)x0;
            if (A.vec && x0 + 4 <= A.w)
            {
                const uint4 q = *reinterpret_cast<const uint4 *>(row);
                const uint32_t bits[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; j++)
                    __builtin_memcpy(&v[i][j], &bits[j], 4);
            }
            else
            {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x0 + j < A.w)
                        v[i][j] = row[j];
            }
        }
    }
    // level 1: 2 x 2 pixels at (y0 / 2, x0 / 2)
    const int64_t w1 = level_extent(A.w, 1), h1 = level_extent(A.h, 1);
    T l1[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
        {
            l1[i][j] = R::cell(v[2 * i][2 * j], v[2 * i][2 * j + 1], v[2 * i + 1][2 * j], v[2 * i + 1][2 * j + 1],
                               x0 + 2 * j + 1 < A.w, y0 + 2 * i + 1 < A.h);
            const int64_t X = x0 / 2 + j, Y = y0 / 2 + i;
            if (X < w1 && Y < h1)
                A.dst[1][(size_t)Y * (size_t)w1 + (size_t)X] = l1[i][j];
        }
    if (A.depth < 2)
        return;
    // level 2: one pixel at (y0 / 4, x0 / 4), kept in LDS for the levels above
    {
        const int64_t w2 = level_extent(A.w, 2), h2 = level_extent(A.h, 2);
        const int64_t X = x0 / 4, Y = y0 / 4;
        const T p = R::cell(l1[0][0], l1[0][1], l1[1][0], l1[1][1], x0 / 2 + 1 < w1, y0 / 2 + 1 < h1);
        if (X < w2 && Y < h2)
            A.dst[2][(size_t)Y * (size_t)w2 + (size_t)X] = p;
        plane[0][ty * 16 + tx] = p;
    }
    // levels 3 .. 6: 8 x 8, 4 x 4, 2 x 2, 1 pixels of the block
    int from = 0;
    for (int k = 3; k <= A.depth; k++)
    {
        __syncthreads();
        const int n = 64 >> k; // the block's side at level k
        if (t < n * n)
        {
            const int lx = t % n, ly = t / n;
            const int64_t wk = level_extent(A.w, k), hk = level_extent(A.h, k);
            const int64_t wp = level_extent(A.w, k - 1), hp = level_extent(A.h, k - 1);
            const int64_t X = (int64_t)blockIdx.x * n + lx, Y = (A.row_a >> k) + (int64_t)blockIdx.y * n + ly;
            const T *s = &plane[from][(2 * ly) * (2 * n) + 2 * lx];
            const T p = R::cell(s[0], s[1], s[2 * n], s[2 * n + 1], 2 * X + 1 < wp, 2 * Y + 1 < hp);
            if (X < wk && Y < hk)
                A.dst[k][(size_t)Y * (size_t)wk + (size_t)X] = p;
            plane[from ^ 1][ly * n + lx] = p;
        }
        from ^= 1;
    }
}

template <class T> struct plain_args
{
    const T *src;     // the level before: its rows from src_row0 on
    int64_t src_row0, src_w, src_h;
    const T *top;     // not NULL: the source row 2 r0 (the pending row)
    T *dst;           // the whole level
    int64_t dst_w, r0, r1;
};

template <class R> __global__ __launch_bounds__(PLAIN_THREADS) void overview_plain(const plain_args<typename R::type> A)
{
    using T = typename R::type;
    const size_t i = (size_t)blockIdx.x * PLAIN_THREADS + threadIdx.x;
    if (i >= (size_t)(A.r1 - A.r0) * (size_t)A.dst_w)
        return;
    const int64_t r = A.r0 + (int64_t)(i / (size_t)A.dst_w), c = (int64_t)(i % (size_t)A.dst_w);
    const bool has_bottom = 2 * r + 1 < A.src_h, has_right = 2 * c + 1 < A.src_w;
    const T *s0 = A.top && r == A.r0 ? A.top : A.src + (size_t)(2 * r - A.src_row0) * (size_t)A.src_w;
    const T *s1 = has_bottom ? A.src + (size_t)(2 * r + 1 - A.src_row0) * (size_t)A.src_w : s0;
    const int64_t c1 = has_right ? 2 * c + 1 : 2 * c;
    A.dst[(size_t)r * (size_t)A.dst_w + (size_t)c] = R::cell(s0[2 * c], s0[c1], s1[2 * c], s1[c1], has_right, has_bottom);
}

} // namespace

struct ochip_ortho_overviews
{
    ochip_ctx *ctx = nullptr;
    int kind = 0;
    bool on_device = false;
    ochip_ov::progress P;
    ochip::dev_blocks mem;         // the pending row; with host levels the device's copies of them too
    void *pending = nullptr;       // one level-0 row
    std::vector<void *> level_dev; // [1 .. levels]: where the kernels write
    std::vector<void *> level_out; // the caller's buffers
};

namespace
{

template <class R> int run_steps(ochip_ortho_overviews *o, const std::vector<step> &steps, int64_t row0, const void *band_dev)
{
    using T = typename R::type;
    ochip_ctx *ctx = o->ctx;
    const progress &P = o->P;
    const T *band = static_cast<const T *>(band_dev);
    for (const step &s : steps)
    {
        if (s.what == step::KEEP)
        {
            OCHIP_HIP(ctx, hipMemcpyAsync(o->pending, band + (size_t)(s.r0 - row0) * (size_t)P.width, (size_t)P.width * 4,
                                          hipMemcpyDeviceToDevice, ctx->stream));
            continue;
        }
        if (s.what == step::FUSED)
        {
            fused_args<T> A{};
            A.src = band, A.src_row0 = row0, A.row_a = s.r0, A.w = P.width, A.h = P.height;
            A.depth = P.levels < FUSED_DEPTH ? P.levels : FUSED_DEPTH;
            A.vec = P.width % 4 == 0 && (uintptr_t)band % 16 == 0;
            for (int k = 1; k <= A.depth; k++)
                A.dst[k] = static_cast<T *>(o->level_dev[k]);
            const int64_t bx = (P.width + 63) / 64, by = (s.r1 - s.r0 + 63) / 64;
            if (bx > 0x7FFFFFFF || by > 65535)
                return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_overviews_feed: %lld x %lld blocks exceed the grid", (long long)bx,
                                  (long long)by);
            hipLaunchKernelGGL(overview_fused<R>, dim3((uint32_t)bx, (uint32_t)by), dim3(FUSED_THREADS), 0, ctx->stream, A);
        }
        else
        {
            plain_args<T> A{};
            if (s.level == 1)
                A.src = band, A.src_row0 = row0;
            else
                A.src = static_cast<const T *>(o->level_dev[s.level - 1]), A.src_row0 = 0;
            A.src_w = P.level_w(s.level - 1), A.src_h = P.level_h(s.level - 1);
            A.top = s.top_pending ? static_cast<const T *>(o->pending) : nullptr;
            A.dst = static_cast<T *>(o->level_dev[s.level]), A.dst_w = P.level_w(s.level), A.r0 = s.r0, A.r1 = s.r1;
            const size_t total = (size_t)(s.r1 - s.r0) * (size_t)A.dst_w, blocks = (total + PLAIN_THREADS - 1) / PLAIN_THREADS;
            if (blocks > 0x7FFFFFFF)
                return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_overviews_feed: %zu pixels of level %d exceed the grid", total, s.level);
            hipLaunchKernelGGL(overview_plain<R>, dim3((uint32_t)blocks), dim3(PLAIN_THREADS), 0, ctx->stream, A);
        }
        if (hipGetLastError() != hipSuccess)
            return ochip_fail(ctx, OCHIP_EHIP, "overview kernel launch failed");
    }
    return OCHIP_OK;
}

} // namespace

extern "C"
{

int ochip_ortho_overviews_levels(int64_t width, int64_t height, int64_t *rows_cols)
{
    if (width < 1 || height < 1)
        return OCHIP_EINVAL;
    const int n = ochip_ov::num_levels(width, height);
    for (int k = 1; k <= n && rows_cols; k++)
        rows_cols[2 * (k - 1)] = ochip_ov::level_extent(height, k), rows_cols[2 * (k - 1) + 1] = ochip_ov::level_extent(width, k);
    return n;
}

int ochip_ortho_overviews_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, void *const *levels, int on_device,
                                 ochip_ortho_overviews **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out || (kind != KIND_RGBA8 && kind != KIND_FLOAT32) || width < 1 || height < 1)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_overviews_create: bad argument (%lld x %lld, kind %d)", (long long)width,
                          (long long)height, kind);
    *out = nullptr;
    const int n = ochip_ov::num_levels(width, height);
    for (int k = 0; k < n; k++)
        if (!levels || !levels[k])
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_overviews_create: %lld x %lld has %d levels, the buffer of level %d is NULL",
                              (long long)width, (long long)height, n, k + 1);
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<ochip_ortho_overviews> o(new ochip_ortho_overviews);
    o->ctx = ctx, o->kind = kind, o->on_device = on_device != 0;
    o->mem.ctx = ctx, o->mem.what = "ochip_ortho_overviews";
    o->P.reset(width, height);
    o->level_dev.assign((size_t)n + 1, nullptr), o->level_out.assign((size_t)n + 1, nullptr);
    bool ok = true;
    if (n > 0)
        ok = (o->pending = o->mem.get((size_t)width * 4)) != nullptr;
    for (int k = 1; k <= n && ok; k++)
    {
        o->level_out[k] = levels[k - 1];
        o->level_dev[k] = on_device ? levels[k - 1] : o->mem.get((size_t)o->P.level_w(k) * (size_t)o->P.level_h(k) * 4);
        ok = o->level_dev[k] != nullptr;
    }
    if (!ok)
    {
        o->mem.release(); // nothing was launched on the blocks
        return OCHIP_ENOMEM;
    }
    *out = o.release();
    return OCHIP_OK;
}

int ochip_ortho_overviews_feed(ochip_ortho_overviews *o, int64_t row0, int64_t rows, const void *band)
{
    if (!o)
        return OCHIP_EINVAL;
    ochip_ctx *ctx = o->ctx;
    if (!band)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_overviews_feed: the band is NULL");
    const std::vector<int64_t> before = o->P.done;
    std::vector<step> steps;
    const std::string refusal = o->P.feed(row0, rows, !ochip_test_hook("overview_per_level"), &steps);
    if (!refusal.empty())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_overviews_feed: %s", refusal.c_str());
    if (steps.empty())
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_scratch scratch{ctx, "ochip_ortho_overviews_feed"};
    const void *band_dev = band;
    if (!o->on_device)
    {
        void *up = nullptr;
        OCHIP_TRY(scratch.upload_bytes(&up, band, (size_t)rows * (size_t)o->P.width * 4, ochip::copy_mode::enqueue));
        band_dev = up;
    }
    OCHIP_TRY(o->kind == KIND_RGBA8 ? run_steps<rgba_rule>(o, steps, row0, band_dev) : run_steps<float_rule>(o, steps, row0, band_dev));
    if (!o->on_device)
    {
        // host levels: the rows this feed completed, then the one wait that also frees the uploaded band
        for (int k = 1; k <= o->P.levels; k++)
            if (o->P.done[k] > before[k])
            {
                const size_t off = (size_t)before[k] * (size_t)o->P.level_w(k) * 4;
                OCHIP_HIP(ctx, hipMemcpyAsync((char *)o->level_out[k] + off, (const char *)o->level_dev[k] + off,
                                              (size_t)(o->P.done[k] - before[k]) * (size_t)o->P.level_w(k) * 4, hipMemcpyDeviceToHost,
                                              ctx->stream));
            }
        if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
            return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ochip_ortho_overviews_feed)");
        scratch.release();
    }
    return OCHIP_OK;
}

int64_t ochip_ortho_overviews_complete_rows(const ochip_ortho_overviews *o, int level)
{
    return o && level >= 1 && level <= o->P.levels ? o->P.done[level] : 0;
}

int ochip_ortho_overviews_finish(ochip_ortho_overviews *o)
{
    if (!o)
        return OCHIP_EINVAL;
    const std::string refusal = o->P.finish();
    if (!refusal.empty())
        return ochip_fail(o->ctx, OCHIP_EINVAL, "ochip_ortho_overviews_finish: %s", refusal.c_str());
    // the levels are the caller's to read from here on
    if (o->P.levels > 0 && ochip_stream_wait(o->ctx, o->ctx->stream) != hipSuccess)
        return ochip_fail(o->ctx, OCHIP_EHIP, "stream wait failed (ochip_ortho_overviews_finish)");
    return OCHIP_OK;
}

void ochip_ortho_overviews_destroy(ochip_ortho_overviews *o)
{
    if (!o)
        return;
    if (!o->mem.empty()) // nothing may still touch the blocks when they go back to the pool
        (void)ochip_stream_wait(o->ctx, o->ctx->stream);
    o->mem.release();
    delete o;
}

} // extern "C"
