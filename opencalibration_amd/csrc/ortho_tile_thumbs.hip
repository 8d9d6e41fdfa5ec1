// Per-tile progress thumbnails of the layer and blend passes on the device (the arithmetic:
// ortho_tile_thumbs.hpp).  One kernel, one launch per band and pass on the context's stream: a lane per slot pixel, consecutive
// lanes consecutive thumbnail x, so a wavefront's loads fall into one row segment of 64 * scale * 4 bytes; blockIdx.x is the
// tile, so the tile's geometry is the same in every lane of a workgroup and a partial tile only shortens the part of its
// slot that reads.  Every slot pixel is written - the thumbnail, then zeros - so the output needs no fill.  No atomics, no LDS.
// A job keeps the band's thumbnails in a block of the context's device pool and a page-locked block of its host pool: enqueue
// launches the kernel and the copy and records an event, wait sleeps on that event alone.
#include "ctx.hpp"
#include "ortho_tile_thumbs.hpp"

#include <cstring>
#include <memory>

namespace
{

using namespace ochip_tt;

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void tile_thumbs(const band B, uint32_t *__restrict__ out)
{
    const uint32_t slot = (uint32_t)B.slot_pixels(), i = blockIdx.y * THREADS + threadIdx.x;
    if (i >= slot)
        return;
    out[(size_t)blockIdx.x * slot + i] = slot_value(B, (int64_t)blockIdx.x, i);
}

} // namespace

struct ochip_tile_thumbs_job
{
    ochip_ctx *ctx = nullptr;
    ochip::dev_blocks mem; // the slots; with host inputs the uploaded band too
    void *host = nullptr;  // page-locked: where the copy lands
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool recorded = false, waited = false;
};

extern "C"
{

int ochip_ortho_tile_thumb_dims(int32_t tw, int32_t th, int32_t *dims3)
{
    if (tw < 1 || th < 1 || tw > MAX_TILE || th > MAX_TILE || !dims3)
        return OCHIP_EINVAL;
    const thumb_dims d = dims_of(tw, th);
    dims3[0] = d.scale, dims3[1] = d.w, dims3[2] = d.h;
    return OCHIP_OK;
}

void ochip_ortho_tile_thumbs_release(ochip_tile_thumbs_job *job)
{
    if (!job)
        return;
    if (!job->waited && !job->mem.empty())
    {
        // nothing may still touch the blocks when they go back to the pools
        if (job->recorded)
            (void)hipEventSynchronize(job->done);
        else if (job->ctx->stream.opened())
            (void)ochip_stream_wait(job->ctx, job->ctx->stream);
    }
    if (job->done)
        (void)hipEventDestroy(job->done);
    job->mem.release();
    ochip_host_free(job->ctx, job->host);
    delete job;
}

int ochip_ortho_tile_thumbs_enqueue(ochip_ctx *ctx, int pass, int32_t cols, int64_t rows, int32_t tile_size, int32_t num_layers,
                                    int on_device, const uint8_t *pixels, const float *weight, ochip_tile_thumbs_job **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_tile_thumbs_enqueue: out is NULL");
    *out = nullptr;
    const std::string why = refusal(pass, cols, rows, tile_size, num_layers, pixels, weight);
    if (!why.empty())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_tile_thumbs: %s", why.c_str());
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    band B{pass, cols, tile_size, num_layers, rows, reinterpret_cast<const uint32_t *>(pixels), pass == PASS_LAYERS ? weight : nullptr};
    struct releaser
    {
        void operator()(ochip_tile_thumbs_job *j) const
        {
            ochip_ortho_tile_thumbs_release(j);
        }
    };
    std::unique_ptr<ochip_tile_thumbs_job, releaser> job(new ochip_tile_thumbs_job);
    job->ctx = ctx, job->mem.ctx = ctx, job->mem.what = "ochip_ortho_tile_thumbs";
    job->bytes = (size_t)B.tiles() * B.slot_pixels() * 4;
    if (!on_device)
    {
        // host inputs: the caller's arrays are theirs again on return
        const size_t plane = (size_t)rows * (size_t)cols, n = pass == PASS_LAYERS ? (size_t)num_layers * plane : plane;
        void *up = nullptr;
        OCHIP_TRY(job->mem.upload_bytes(&up, pixels, n * 4, B.weight ? ochip::copy_mode::enqueue : ochip::copy_mode::enqueue_wait));
        B.pixels = static_cast<const uint32_t *>(up);
        if (B.weight)
        {
            OCHIP_TRY(job->mem.upload_bytes(&up, weight, n * 4, ochip::copy_mode::enqueue_wait));
            B.weight = static_cast<const float *>(up);
        }
    }
    uint32_t *slots = static_cast<uint32_t *>(job->mem.get(job->bytes));
    if (!slots)
        return OCHIP_ENOMEM;
    OCHIP_TRY(ochip_host_alloc(ctx, job->bytes, &job->host));
    OCHIP_HIP(ctx, hipEventCreateWithFlags(&job->done, hipEventBlockingSync | hipEventDisableTiming));
    const uint32_t blocks_per_slot = (uint32_t)((B.slot_pixels() + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(tile_thumbs, dim3((uint32_t)B.tiles(), blocks_per_slot), dim3(THREADS), 0, ctx->stream, B, slots);
    if (hipGetLastError() != hipSuccess)
        return ochip_fail(ctx, OCHIP_EHIP, "tile thumbnail kernel launch failed");
    OCHIP_HIP(ctx, hipMemcpyAsync(job->host, slots, job->bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, hipEventRecord(job->done, ctx->stream));
    job->recorded = true;
    *out = job.release();
    return OCHIP_OK;
}

int ochip_ortho_tile_thumbs_wait(ochip_tile_thumbs_job *job, const uint8_t **thumbs, uint64_t *bytes)
{
    if (!job)
        return OCHIP_EINVAL;
    if (!job->waited)
    {
        OCHIP_HIP(job->ctx, hipEventSynchronize(job->done));
        job->waited = true;
    }
    if (thumbs)
        *thumbs = static_cast<const uint8_t *>(job->host);
    if (bytes)
        *bytes = job->bytes;
    return OCHIP_OK;
}

int ochip_ortho_tile_thumbs(ochip_ctx *ctx, int pass, int32_t cols, int64_t rows, int32_t tile_size, int32_t num_layers, int on_device,
                            const uint8_t *pixels, const float *weight, uint8_t *thumbs_out)
{
    if (!thumbs_out || (uintptr_t)thumbs_out % 4)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_ortho_tile_thumbs: the thumbnails' array is NULL or not 4-byte aligned");
    if (ctx)
    {
        ochip_tile_thumbs_job *job = nullptr;
        OCHIP_TRY(ochip_ortho_tile_thumbs_enqueue(ctx, pass, cols, rows, tile_size, num_layers, on_device, pixels, weight, &job));
        const int rc = ochip_ortho_tile_thumbs_wait(job, nullptr, nullptr);
        if (rc == OCHIP_OK)
            std::memcpy(thumbs_out, job->host, job->bytes);
        ochip_ortho_tile_thumbs_release(job);
        return rc;
    }
    // the CPU route, over host inputs
    const std::string why = on_device ? std::string("inputs on the device need a device context")
                                      : refusal(pass, cols, rows, tile_size, num_layers, pixels, weight);
    if (!why.empty())
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_ortho_tile_thumbs: %s", why.c_str());
    const band B{pass, cols, tile_size, num_layers, rows, reinterpret_cast<const uint32_t *>(pixels), pass == PASS_LAYERS ? weight : nullptr};
    cpu_route(B, reinterpret_cast<uint32_t *>(thumbs_out));
    return OCHIP_OK;
}

} // extern "C"
