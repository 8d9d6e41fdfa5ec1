// The load stage's image thumbnails on the device (rules: thumbnail.hpp).
//
//   thumb_table_fill   once per context: lab_word() of all 2^24 BGR codes, so that no image pays for the cube roots
//   thumb_rows         per source row: the row's window through LDS (16-byte loads), its pixels' Lab gathered from the
//                      table, then one thread per (destination column, channel) walks its horizontal taps in table order
//   thumb_cols         per destination value the vertical taps in table order, rounding, and Lab -> R G B per pixel
//
// Every float sum is one thread's chain in the table's order: no tree, no atomics.  The integer path (n x n cells) runs
// through the same two kernels with integer sums.
#include "area_table.hpp"
#include "ctx.hpp"
#include "thumbnail.hpp"

#include <algorithm>
#include <vector>

namespace
{

constexpr int THREADS = 256;
constexpr int STAGE_PX = 4096;                        // source pixels of one row that a workgroup stages
constexpr int STAGE_VEC = (STAGE_PX * 3 + 15) / 16 + 2; // 16-byte words: the window and its misalignment at either end
constexpr int COLS_PX = 64, COLS_THREADS = COLS_PX * 3;
constexpr uint32_t CODES = 1u << 24;

__global__ __launch_bounds__(THREADS) void thumb_table_fill(const ochip_ol::lab_tables *__restrict__ T, uint32_t *__restrict__ table)
{
    const uint32_t code = blockIdx.x * THREADS + threadIdx.x; // the grid holds exactly CODES threads
    table[code] = ochip_th::lab_word(*T, code);
}

__global__ __launch_bounds__(THREADS) void thumb_table_read(const uint32_t *__restrict__ table, const uint32_t *__restrict__ codes,
                                                            size_t n, uint32_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < n)
        out[i] = table[codes[i] & (CODES - 1)];
}

// one axis of the resize: destination d covers source [first[d], first[d] + count[d]); general path: its weights at
// alpha[off[d] ..]
struct axis_args
{
    const int *first, *count, *off;
    const float *alpha;
};

struct rows_args
{
    const uint8_t *src; // the chunk's images, [B][h][w][3]
    size_t src_bytes;   // their size: no load leaves [src, src + src_bytes)
    int w, h, dw;
    uint32_t nseg;
    const int *seg; // [nseg + 1]: segment s holds destination columns [seg[s], seg[s + 1]), whose window is <= STAGE_PX
    axis_args x;
    const uint32_t *table;
    uint32_t *sums; // [B][h][dw][3]: float bits (general) or integer sums
};

template <bool INTEGER> __global__ __launch_bounds__(THREADS) void thumb_rows(rows_args A)
{
    __shared__ uint4 raw[STAGE_VEC];
    __shared__ uint32_t lab[STAGE_PX];
    const uint32_t s = blockIdx.x % A.nseg, line = blockIdx.x / A.nseg; // line = image * h + row
    const int x0 = A.seg[s], x1 = A.seg[s + 1];
    const int p0 = A.x.first[x0], np = A.x.first[x1 - 1] + A.x.count[x1 - 1] - p0; // 1 <= np <= STAGE_PX (the host's check)
    const uintptr_t lo = (uintptr_t)A.src, hi = lo + A.src_bytes;
    const uintptr_t g = lo + ((size_t)line * (size_t)A.w + (size_t)p0) * 3;
    const uintptr_t a = g & ~(uintptr_t)15;
    const uint32_t lead = (uint32_t)(g - a), nvec = (lead + (uint32_t)np * 3 + 15) >> 4; // <= STAGE_VEC
    for (uint32_t j = threadIdx.x; j < nvec; j += THREADS)
    {
        const uintptr_t addr = a + 16 * (uintptr_t)j;
        uint4 v;
        if (addr >= lo && addr + 16 <= hi)
            v = *reinterpret_cast<const uint4 *>(addr);
        else
        {
            // the 16 bytes straddle an end of the buffer: byte by byte, zeros outside
            uint32_t w4[4] = {0, 0, 0, 0};
            for (int b = 0; b < 16; b++)
                if (addr + b >= lo && addr + b < hi)
                    w4[b >> 2] |= (uint32_t) * reinterpret_cast<const uint8_t *>(addr + b) << (8 * (b & 3));
            v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
        raw[j] = v;
    }
    __syncthreads();
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(raw) + lead;
    for (int p = threadIdx.x; p < np; p += THREADS)
    {
        const uint32_t code = (uint32_t)bytes[3 * p] | (uint32_t)bytes[3 * p + 1] << 8 | (uint32_t)bytes[3 * p + 2] << 16;
        lab[p] = A.table[code];
    }
    __syncthreads();
    const int chains = (x1 - x0) * 3;
    for (int q = threadIdx.x; q < chains; q += THREADS)
    {
        const int dx = x0 + q / 3, c = q % 3, shift = 8 * c;
        const int s0 = A.x.first[dx] - p0, count = A.x.count[dx]; // s0 >= 0, s0 + count <= np
        uint32_t out;
        if (INTEGER)
        {
            out = 0;
            for (int k = 0; k < count; k++)
                out += lab[s0 + k] >> shift & 255u;
        }
        else
        {
            const float *al = A.x.alpha + A.x.off[dx];
            float acc = 0.0f;
            for (int k = 0; k < count; k++)
                acc = ochip_th::tap(acc, (float)(lab[s0 + k] >> shift & 255u), al[k]);
            out = __float_as_uint(acc);
        }
        A.sums[((size_t)line * (size_t)A.dw + (size_t)dx) * 3 + c] = out;
    }
}

struct cols_args
{
    const uint32_t *sums; // [B][h][dw][3]
    int h, dw, dh, n;
    uint32_t pixels; // B * dh * dw
    axis_args y;
    const int *xcount;
    const ochip_ol::lab_tables *T;
    uint8_t *out; // [B][dh][dw][3] R G B
};

template <bool INTEGER> __global__ __launch_bounds__(COLS_THREADS) void thumb_cols(cols_args A)
{
    __shared__ uint8_t lab8[COLS_THREADS];
    const uint32_t P = blockIdx.x * COLS_PX + threadIdx.x / 3;
    const int c = threadIdx.x % 3;
    uint8_t v = 0;
    if (P < A.pixels)
    {
        const uint32_t per = (uint32_t)A.dh * (uint32_t)A.dw;
        const uint32_t img = P / per, r = P % per;
        const int dy = (int)(r / (uint32_t)A.dw), dx = (int)(r % (uint32_t)A.dw);
        const size_t stride = (size_t)A.dw * 3;
        const int y0 = A.y.first[dy], count = A.y.count[dy]; // y0 + count <= h
        const uint32_t *col = A.sums + ((size_t)img * (size_t)A.h + (size_t)y0) * stride + (size_t)dx * 3 + c;
        if (INTEGER)
        {
            uint32_t sum = 0;
            for (int k = 0; k < count; k++)
                sum += col[(size_t)k * stride];
            v = ochip_th::cell_value(sum, A.xcount[dx], count, A.n);
        }
        else
        {
            const float *be = A.y.alpha + A.y.off[dy];
            float acc = 0.0f;
            for (int k = 0; k < count; k++)
                acc = ochip_th::tap(acc, __uint_as_float(col[(size_t)k * stride]), be[k]);
            v = ochip_th::round8(acc);
        }
    }
    lab8[threadIdx.x] = v;
    __syncthreads();
    const uint32_t Q = blockIdx.x * COLS_PX + threadIdx.x;
    if (threadIdx.x < COLS_PX && Q < A.pixels)
    {
        uint8_t rgb[3];
        ochip_th::rgb_from_lab8(*A.T, &lab8[3 * threadIdx.x], rgb);
        A.out[(size_t)Q * 3] = rgb[0], A.out[(size_t)Q * 3 + 1] = rgb[1], A.out[(size_t)Q * 3 + 2] = rgb[2];
    }
}

// the table of all BGR codes and the conversion's own tables, on first use
int ensure_lab_table(ochip_ctx *ctx)
{
    if (ctx->lab_table_dev)
        return OCHIP_OK;
    ochip_ol::lab_tables tables;
    ochip_ol::lab_tables_build(&tables);
    auto *mem = new ochip::dev_blocks(ctx, "the thumbnail pass's Lab table");
    ochip_ol::lab_tables *d_tables = nullptr;
    uint32_t *d_table = nullptr;
    int rc = mem->upload(&d_tables, &tables, 1, ochip::copy_mode::enqueue_wait);
    if (rc == OCHIP_OK)
        rc = mem->alloc<uint32_t>(&d_table, CODES);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (rc == OCHIP_OK && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess))
        rc = ochip_fail(ctx, OCHIP_EHIP, "event creation failed (thumbnail table)");
    if (rc == OCHIP_OK)
    {
        (void)hipEventRecord(e0, ctx->stream);
        hipLaunchKernelGGL(thumb_table_fill, dim3(CODES / THREADS), dim3(THREADS), 0, ctx->stream, d_tables, d_table);
        (void)hipEventRecord(e1, ctx->stream);
        if (hipGetLastError() != hipSuccess || ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
            rc = ochip_fail(ctx, OCHIP_EHIP, "the thumbnail pass's table fill failed");
        else
            (void)hipEventElapsedTime(&ctx->lab_table_fill_ms, e0, e1);
    }
    if (e0)
        (void)hipEventDestroy(e0);
    if (e1)
        (void)hipEventDestroy(e1);
    if (rc != OCHIP_OK)
    {
        mem->release();
        delete mem;
        return rc;
    }
    ctx->lab_table_mem = mem;
    ctx->lab_tables_dev = d_tables;
    ctx->lab_table_dev = d_table;
    return OCHIP_OK;
}

// the host's description of one axis; false: a table that the kernels' indexing does not cover
bool make_axis(const ochip_th::plan &P, int ssize, int dsize, std::vector<int> *first, std::vector<int> *count, area_tab *tab)
{
    first->resize(dsize), count->resize(dsize);
    if (P.n > 0)
    {
        for (int d = 0; d < dsize; d++)
            ochip_th::cell_range(d, P.n, ssize, &(*first)[d], &(*count)[d]);
    }
    else
    {
        *tab = area_table(ssize, dsize, P.inv_scale);
        for (int d = 0; d < dsize; d++)
        {
            const int k0 = tab->off[d], nk = tab->off[d + 1] - k0;
            if (nk < 1)
                return false;
            for (int k = 1; k < nk; k++) // a cell's taps are consecutive pixels
                if (tab->si[k0 + k] != tab->si[k0] + k)
                    return false;
            (*first)[d] = tab->si[k0], (*count)[d] = nk;
        }
    }
    for (int d = 0; d < dsize; d++)
        if ((*count)[d] < 1 || (*first)[d] < 0 || (*first)[d] + (*count)[d] > ssize ||
            (d && ((*first)[d] < (*first)[d - 1] || (*first)[d] + (*count)[d] < (*first)[d - 1] + (*count)[d - 1])))
            return false; // (cells advance: a segment's window runs from its first cell's first pixel to its last cell's last)
    return true;
}

} // namespace

extern "C"
{

int ochip_thumbnail_size(int width, int height, int32_t *rows, int32_t *cols)
{
    ochip_th::plan P;
    if (!rows || !cols || ochip_th::make_plan(width, height, &P) != ochip_th::SIZE_OK)
        return OCHIP_EINVAL;
    *rows = P.rows, *cols = P.cols;
    return OCHIP_OK;
}

int ochip_debug_lab_table(ochip_ctx *ctx, const uint32_t *codes, size_t n, uint32_t *out, float *fill_ms)
{
    if (!ctx || (n && (!codes || !out)))
        return ctx ? ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_lab_table: bad argument") : OCHIP_EINVAL;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    OCHIP_TRY(ensure_lab_table(ctx));
    if (fill_ms)
        *fill_ms = ctx->lab_table_fill_ms;
    if (n == 0)
        return OCHIP_OK;
    ochip::dev_scratch mem{ctx, "ochip_debug_lab_table"};
    uint32_t *d_codes = nullptr, *d_out = nullptr;
    OCHIP_TRY(mem.upload(&d_codes, codes, n, ochip::copy_mode::enqueue_wait));
    OCHIP_TRY(mem.alloc<uint32_t>(&d_out, n));
    hipLaunchKernelGGL(thumb_table_read, dim3((uint32_t)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, ctx->stream,
                       ctx->lab_table_dev, d_codes, n, d_out);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "thumb_table_read launch failed");
    OCHIP_HIP(ctx, hipMemcpyAsync(out, d_out, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ochip_debug_lab_table)");
    mem.release();
    return OCHIP_OK;
}

int ochip_image_thumbnails(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                           int images_on_device, uint8_t *rgb_out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    ochip_th::plan P;
    const int bad = ochip_th::make_plan(width, height, &P);
    if (bad)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_image_thumbnails: %s", ochip_th::size_error(bad));
    if (n_images && (!images_bgr || !rgb_out))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_image_thumbnails: a NULL image or output pointer");
    if (n_images == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    OCHIP_TRY(ensure_lab_table(ctx));

    std::vector<int> xfirst, xcount, yfirst, ycount, seg;
    area_tab tx, ty;
    if (!make_axis(P, width, P.cols, &xfirst, &xcount, &tx) || !make_axis(P, height, P.rows, &yfirst, &ycount, &ty))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_image_thumbnails: unexpected resize table for %d x %d", width, height);
    // segments of destination columns whose source window fits the staging buffer
    for (int x0 = 0; x0 < P.cols;)
    {
        seg.push_back(x0);
        int x1 = x0 + 1;
        if (xcount[x0] > STAGE_PX)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_image_thumbnails: a cell of %d source columns exceeds the staging window",
                              xcount[x0]);
        while (x1 < P.cols && xfirst[x1] + xcount[x1] - xfirst[x0] <= STAGE_PX)
            x1++;
        x0 = x1;
    }
    seg.push_back(P.cols);
    const uint32_t nseg = (uint32_t)seg.size() - 1;

    const size_t src_bytes = (size_t)width * height * 3, dst_bytes = (size_t)P.rows * P.cols * 3;
    const size_t sums_bytes = (size_t)height * P.cols * 3 * 4;
    // images per chunk: 64 MB of row sums, 256 MB of uploaded source, and grids below 2^31 blocks
    size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / sums_bytes);
    if (!images_on_device)
        chunk = std::max<size_t>(1, std::min(chunk, ((size_t)256 << 20) / src_bytes));
    chunk = std::min(chunk, (size_t)0x7fffffff / ((size_t)nseg * height));
    chunk = std::min(chunk, (size_t)0x7fffffff / ((size_t)P.rows * P.cols));
    chunk = std::min<size_t>(chunk, n_images);

    constexpr auto WAIT = ochip::copy_mode::enqueue_wait;
    ochip::dev_scratch mem{ctx, "ochip_image_thumbnails"};
    int *d_seg, *d_xfirst, *d_xcount, *d_yfirst, *d_ycount, *d_xoff = nullptr, *d_yoff = nullptr;
    float *d_xal = nullptr, *d_yal = nullptr;
    uint8_t *d_src = nullptr, *d_out = nullptr;
    uint32_t *d_sums = nullptr;
    OCHIP_TRY(mem.upload(&d_seg, seg, WAIT));
    OCHIP_TRY(mem.upload(&d_xfirst, xfirst, WAIT));
    OCHIP_TRY(mem.upload(&d_xcount, xcount, WAIT));
    OCHIP_TRY(mem.upload(&d_yfirst, yfirst, WAIT));
    OCHIP_TRY(mem.upload(&d_ycount, ycount, WAIT));
    if (P.n == 0)
    {
        OCHIP_TRY(mem.upload(&d_xoff, tx.off, WAIT));
        OCHIP_TRY(mem.upload(&d_xal, tx.alpha, WAIT));
        OCHIP_TRY(mem.upload(&d_yoff, ty.off, WAIT));
        OCHIP_TRY(mem.upload(&d_yal, ty.alpha, WAIT));
    }
    if (!images_on_device)
        OCHIP_TRY(mem.alloc<uint8_t>(&d_src, chunk * src_bytes));
    OCHIP_TRY(mem.alloc<uint32_t>(&d_sums, chunk * sums_bytes / 4));
    OCHIP_TRY(mem.alloc<uint8_t>(&d_out, chunk * dst_bytes));

    for (size_t i0 = 0; i0 < n_images; i0 += chunk)
    {
        const size_t B = std::min<size_t>(chunk, n_images - i0);
        const uint8_t *src = images_bgr + i0 * src_bytes;
        if (!images_on_device)
        {
            OCHIP_HIP(ctx, hipMemcpyAsync(d_src, src, B * src_bytes, hipMemcpyHostToDevice, ctx->stream));
            src = d_src;
        }
        rows_args R{};
        R.src = src, R.src_bytes = B * src_bytes;
        R.w = width, R.h = height, R.dw = P.cols;
        R.nseg = nseg, R.seg = d_seg;
        R.x = axis_args{d_xfirst, d_xcount, d_xoff, d_xal};
        R.table = ctx->lab_table_dev;
        R.sums = d_sums;
        cols_args C{};
        C.sums = d_sums;
        C.h = height, C.dw = P.cols, C.dh = P.rows, C.n = P.n;
        C.pixels = (uint32_t)(B * P.rows * P.cols);
        C.y = axis_args{d_yfirst, d_ycount, d_yoff, d_yal};
        C.xcount = d_xcount;
        C.T = static_cast<const ochip_ol::lab_tables *>(ctx->lab_tables_dev);
        C.out = d_out;
        const dim3 rgrid((uint32_t)(B * height * nseg)), cgrid((C.pixels + COLS_PX - 1) / COLS_PX);
        if (P.n > 0)
        {
            hipLaunchKernelGGL(thumb_rows<true>, rgrid, dim3(THREADS), 0, ctx->stream, R);
            hipLaunchKernelGGL(thumb_cols<true>, cgrid, dim3(COLS_THREADS), 0, ctx->stream, C);
        }
        else
        {
            hipLaunchKernelGGL(thumb_rows<false>, rgrid, dim3(THREADS), 0, ctx->stream, R);
            hipLaunchKernelGGL(thumb_cols<false>, cgrid, dim3(COLS_THREADS), 0, ctx->stream, C);
        }
        if (hipGetLastError() != hipSuccess)
            return ochip_fail(ctx, OCHIP_EHIP, "thumbnail kernel launch failed");
        OCHIP_HIP(ctx, hipMemcpyAsync(rgb_out + i0 * dst_bytes, d_out, B * dst_bytes, hipMemcpyDeviceToHost, ctx->stream));
        // the next chunk reuses the scratch, and the caller's source may go once this returns
        if (ochip_stream_wait(ctx, ctx->stream) != hipSuccess)
            return ochip_fail(ctx, OCHIP_EHIP, "stream wait failed (ochip_image_thumbnails)");
    }
    mem.release();
    return OCHIP_OK;
}

} // extern "C"
