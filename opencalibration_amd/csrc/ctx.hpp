// Internal context of libochip.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ochip.h"
#include "env.hpp"

struct ochip_profile_slot
{
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_list;
    uint64_t launches = 0;
    double total_ms = 0;
};

namespace ochip
{
struct dev_blocks;
}

// A context's compute stream, opened by the first use that needs a hipStream_t.  A process has a handful of hardware queues
// per stream priority and the runtime hands a stream its queue when it is created: a context that only fills a gap of the
// sibling list, or only owns pools, opens none and takes no share of a queue.  (A context belongs to one thread at a time,
// so does this.)  If the stream cannot be created the error stays here and ochip_stream_wait - where every call on a
// context ends - reports it.
struct ochip_lazy_stream
{
    hipStream_t s = nullptr;
    int device = 0;
    int priority = -1; // -1: the default priority, 0: the lowest, 1: the highest (ochip_ctx_set_priority)
    hipError_t error = hipSuccess;

    ochip_lazy_stream() = default;
    ochip_lazy_stream(const ochip_lazy_stream &) = delete;
    ochip_lazy_stream &operator=(const ochip_lazy_stream &) = delete;
    bool opened() const
    {
        return s != nullptr;
    }
    operator hipStream_t()
    {
        if (!s)
            open();
        return s;
    }
    void open(); // ctx.hip
};

namespace ochip
{
struct akaze_tables;

// The untyped core of dev_array: one device allocation that only ever grows, and the context's list of them.
struct dev_array_mem
{
    dev_array_mem() = default;
    dev_array_mem(const dev_array_mem &) = delete;
    dev_array_mem &operator=(const dev_array_mem &) = delete;
    void release(); // hipFree, for ochip_ctx_destroy alone (it walks ochip_ctx::dev_arrays)

  protected:
    void *mem = nullptr;
    size_t bytes = 0;
    bool listed = false; // in ctx->dev_arrays, from the first allocation on
    int grow(ochip_ctx *ctx, size_t want); // ctx.hip
};

// A device array that lives as long as its context and only ever grows (a reservation reuses it instead of hipFree /
// hipMalloc, which synchronise the whole device and would stall the other contexts' streams).  ensure(ctx, n) makes room for
// n elements: nothing when n <= capacity, else the old block is freed and one of n elements plus a quarter plus 4 KB taken.
// The CONTENTS DO NOT SURVIVE growth: whoever calls ensure fills the array afterwards (fp4_valid = 0 on a reservation, the
// dirty flags of the image tables and the rays).  Converts to T * for kernel launches and copies; as<U>() is the typed
// view of a byte array that packs tables or holds a struct private to one file.  Freed by ochip_ctx_destroy, not by a
// destructor: the context is deleted after its streams, the arrays go before the pools.
template <class T> struct dev_array : dev_array_mem
{
    size_t capacity = 0; // elements

    int ensure(ochip_ctx *ctx, size_t n)
    {
        if (n <= capacity)
            return OCHIP_OK;
        const int rc = grow(ctx, n * sizeof(T));
        capacity = bytes / sizeof(T);
        return rc;
    }
    operator T *() const
    {
        return static_cast<T *>(mem);
    }
    template <class U> U *as() const
    {
        return static_cast<U *>(mem);
    }
};

// Who filled the RANSAC scratch last: ochip_edge_lists reads what ochip_ransac_homography_batch_sorted left there.
enum class ransac_writer
{
    nothing,
    homography_batch,
    homography_batch_sorted,
    refit,
    epipolar
};

// Device state of the RANSAC entries (ransac.hip), T = correspondences of the batch.  The homography routes and the epipolar
// one keep different structs in `jobs` and `corr`, hence bytes and a typed view at the use.
struct ransac_scratch
{
    dev_array<unsigned char> jobs;  // [n_jobs] ochip_ransac_job, or the epipolar job
    dev_array<unsigned char> corr;  // [T] ochip_ransac_match, or 6 doubles (the two rays)
    dev_array<uint32_t> prosac;     // [T] PROSAC order
    dev_array<uint32_t> eval_order; // [eval_total]
    dev_array<double> coords;       // [T][8]
    dev_array<uint8_t> flags;       // [T][2] homography, [T][5] epipolar
    dev_array<double> lu;           // [n_jobs][81] LU workspaces
    dev_array<unsigned char> out;   // [n_jobs] ochip_ransac_result, then [T] inlier flags
    ransac_writer last = ransac_writer::nothing;

    struct outputs
    {
        ochip_ransac_result *results;
        uint8_t *inliers;
    };
    outputs outputs_of(uint32_t n_jobs) const
    {
        ochip_ransac_result *r = out.as<ochip_ransac_result>();
        return {r, reinterpret_cast<uint8_t *>(r + n_jobs)};
    }
    // Room for a batch of `who`, which becomes the last writer; a refit (flags_per_corr == 0) has no orders and no flags.
    int ensure(ochip_ctx *ctx, ransac_writer who, uint32_t n_jobs, size_t job_bytes, uint64_t T, size_t corr_bytes, uint64_t eval_total,
               unsigned flags_per_corr); // ransac.hip
};
} // namespace ochip

struct ochip_ctx
{
    int device = 0;
    ochip_lazy_stream stream;         // compute stream: every kernel of the hot path is launched here
    hipStream_t copy_stream = nullptr; // created on first use (ochip_copy_stream), not with the context
    std::vector<hipStream_t> retired_streams; // replaced by ochip_ctx_set_priority
    int stream_priority = -1; // what ochip_ctx_set_priority last set (-1: the default stream)
    hipEvent_t sync_event = nullptr;  // ochip_stream_wait: a blocking-sync event (created on first use)
    bool blocking_wait = true;        // OCHIP_BLOCKING_SYNC=0: let the runtime poll instead
    std::string error;
    hipDeviceProp_t prop{};

    // descriptor arena: [total][16] u32, image i at img_off[i] with img_n[i] descriptors
    ochip::dev_array<uint32_t> desc_dev;
    uint64_t desc_capacity = 0, desc_used = 0;
    uint32_t n_images = 0;
    std::vector<uint64_t> img_off;
    std::vector<uint32_t> img_n;
    std::vector<uint8_t> img_set;
    ochip::dev_array<uint64_t> img_off_dev;
    ochip::dev_array<uint32_t> img_n_dev;
    bool img_tables_dirty = true; // ochip_upload_image_tables

    // keypoint store, same indexing as the descriptor arena: pixel xy, owning image, unit rays
    ochip::dev_array<double> kp_xy_dev, rays_dev;
    ochip::dev_array<uint32_t> kp_image_dev;
    ochip::dev_array<double> models_dev; // [n_images][8]: f, ppx, ppy, k1, k2, k3, p1, p2
    std::vector<uint8_t> kp_set;
    bool rays_dirty = false;
    bool kp_store_ready = false; // keypoint buffers sized for the current reservation

    // match scratch
    ochip::dev_array<ochip_pair> pairs_dev;
    ochip::dev_array<uint64_t> out_off_dev;
    ochip::dev_array<ochip_match> match_out_dev;
    uint64_t match_out_total = 0;
    // ochip_match_sort (match_sort.hip): per pair the matches that pass the ratio test as (count << 32 | query) records at the
    // pair's offset, in match_features_subset's output order; the pairs' offsets and match counts (ms_seg_dev packs three
    // tables: [n] u32 begin, [n] u32 end, [n] ochip_pair)
    ochip::dev_array<unsigned long long> ms_recs_dev;
    ochip::dev_array<unsigned char> ms_seg_dev, ms_flag_dev;
    uint32_t ms_pairs = 0;
    // symmetric pairs of a match launch: job table (match.hip's sym_job), column partials
    ochip::dev_array<unsigned char> sym_jobs_dev;
    ochip::dev_array<uint2> sym_part_dev;
    // operands of the matrix-core matcher (match.hip, hamming_2nn_mfma_kernel), same indexing as the descriptor arena: the
    // descriptor's 512 bits as FP4 values 0 / 1 (256 bytes = 16 uint4), (512 - popcount) * 8192 as a float, the popcount;
    // features [0, fp4_valid) are expanded, the rest is done by the next match launch
    ochip::dev_array<uint4> desc_fp4_dev;
    ochip::dev_array<float> desc_negpop_dev;
    ochip::dev_array<uint32_t> desc_pop_dev;
    uint64_t fp4_valid = 0;

    // device state of the RANSAC entries, and which of them wrote it last
    ochip::ransac_scratch ransac;

    // every dev_array above that holds memory (dev_array_mem::grow lists it): what ochip_ctx_destroy frees
    std::vector<ochip::dev_array_mem *> dev_arrays;

    // page-locked host blocks handed out by ochip_host_alloc (live) and recycled ones (pool)
    std::vector<std::pair<void *, size_t>> pinned_live, pinned_pool;
    // recycled device blocks for per-call temporaries (hipMalloc / hipFree are slow and synchronising)
    std::vector<std::pair<void *, size_t>> dev_pool;

    ochip_profile_slot prof[OCHIP_K_COUNT];
    // descriptor distances the match launches computed / delivered since the last profile reset (a pair matched in both
    // directions from one pass computes its n1 x n2 distances once and delivers them twice)
    uint64_t match_computed = 0, match_delivered = 0;
    // fp64 multiply-adds x 2 the Cholesky factorisations of the relax solves issued on the matrix cores (panel and
    // trailing-update GEMMs over the rows inside the block envelope) since the last profile reset
    double relax_mfma_flops = 0;
    // roofline bookkeeping since the last profile reset: RANSAC loop trips x correspondences of their job (an upper bound of the
    // (hypothesis, correspondence) errors evaluated: the SPRT exit of ransac.cpp:197-200 leaves a hypothesis early), residual
    // blocks the relax evaluation kernels processed with / without Jacobians
    uint64_t ransac_hyp_corr = 0, relax_blocks_jac = 0, relax_blocks_cost = 0;
    uint64_t relax_system_bytes = 0, relax_system_dense_bytes = 0, relax_system_unknowns = 0; // largest reduced system held (relax_lm.hip)

    // sibling contexts on the same device (own streams, scratch and pools) handed out by ochip_ctx_sibling so
    // that independent batches can be in flight at once; owned by this context
    std::vector<ochip_ctx *> siblings;
    std::mutex siblings_mutex; // ochip_ctx_sibling may be called from concurrent runner threads (RelaxStage's group runners)

    // chunks of ochip_akaze_* on this context whose first host read-back (the candidate counts, after the scale space and
    // the detector) has arrived: ochip_akaze_progress, for a caller that starts its launch sequences out of step
    std::atomic<uint64_t> akaze_readbacks{0};

    // thumbnail.hip: the 8-bit Lab of all 2^24 BGR codes (64 MB, L | a << 8 | b << 16) and the conversion's tables, filled on
    // the first thumbnail call; lab_table_mem owns both blocks
    ochip::dev_blocks *lab_table_mem = nullptr;
    uint32_t *lab_table_dev = nullptr;
    void *lab_tables_dev = nullptr; // ochip_ol::lab_tables
    float lab_table_fill_ms = 0;    // the fill kernel's time (ochip_debug_lab_table)

    // akaze.hip: the tables a chunk's launches read that depend on the image shape alone, kept from chunk to chunk
    ochip::akaze_tables *akaze_tabs = nullptr;
    void (*akaze_tabs_destroy)(ochip::akaze_tables *) = nullptr;

    // what the host library keeps with the context (ochip_ctx_attachment: the extraction slots of host/extract_slots.hpp)
    void *attachment = nullptr;
    void (*attachment_destroy)(void *) = nullptr;
};


// Wait for a stream without spinning: an event created with hipEventBlockingSync puts the waiting host thread to sleep
// whatever scheduling flags the device's primary context was created with (hipSetDeviceFlags is refused once another
// library - PyTorch, RCCL - has initialised the device, which is exactly the multi-GPU case).  The threads that wait
// here would otherwise eat the CPU quota the OpenMP teams of the host phases need.
inline hipError_t ochip_stream_wait(ochip_ctx *ctx, hipStream_t st)
{
    if (ctx->stream.error != hipSuccess)
        return ctx->stream.error;
    if (!ctx->blocking_wait)
        return hipStreamSynchronize(st);
    if (!ctx->sync_event)
    {
        const hipError_t e = hipEventCreateWithFlags(&ctx->sync_event, hipEventBlockingSync | hipEventDisableTiming);
        if (e != hipSuccess)
            return e;
    }
    const hipError_t e = hipEventRecord(ctx->sync_event, st);
    return e != hipSuccess ? e : hipEventSynchronize(ctx->sync_event);
}

// The context's second stream, for a copy that should run beside the context's own kernels: created on first use.
inline hipError_t ochip_copy_stream(ochip_ctx *ctx, hipStream_t *out)
{
    hipError_t e = hipSuccess;
    if (!ctx->copy_stream)
        e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    *out = ctx->copy_stream;
    return e;
}

int ochip_fail(ochip_ctx *ctx, int code, const char *fmt, ...);
int ochip_ensure_keypoint_store(ochip_ctx *ctx, size_t n_keypoints, size_t n_images); // kp_xy, rays, kp_image, models
int ochip_upload_image_tables(ochip_ctx *ctx); // if img_tables_dirty: enqueue the copies of img_off / img_n, clear the flag
void *ochip_pool_get(ochip_ctx *ctx, size_t bytes, size_t *got);          // device block from the pool (or hipMalloc); nullptr on failure
void ochip_pool_put(ochip_ctx *ctx, void *p, size_t bytes);              // hand it back (kept for reuse, freed with the context)
void ochip_prof_begin(ochip_ctx *ctx, int kid, hipEvent_t *start, hipEvent_t *stop);
void ochip_prof_end(ochip_ctx *ctx, int kid, hipEvent_t start, hipEvent_t stop);

#define OCHIP_HIP(ctx, call)                                                                                           \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e__ = (call);                                                                                       \
        if (e__ != hipSuccess)                                                                                         \
            return ochip_fail((ctx), OCHIP_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,    \
                              __LINE__);                                                                               \
    } while (0)

// return a failed step's code (its message is set); with the blocks of a call in a dev_scratch an early return is safe
#define OCHIP_TRY(call)                                                                                                \
    do                                                                                                                 \
    {                                                                                                                  \
        const int rc__ = (call);                                                                                       \
        if (rc__ != OCHIP_OK)                                                                                          \
            return rc__;                                                                                               \
    } while (0)

namespace ochip
{
// How dev_blocks::upload copies into the block it takes: enqueue on ctx->stream and leave the wait to the caller, enqueue and
// wait (the source may be reused on return), or a blocking hipMemcpy.
enum class copy_mode
{
    enqueue,
    enqueue_wait,
    blocking
};

// Device blocks taken from the context's pool and handed back together.  The only user of ochip_pool_get / ochip_pool_put:
// an object that keeps device arrays holds one and releases it in its destroy; a call's temporaries use dev_scratch.
struct dev_blocks
{
    ochip_ctx *ctx = nullptr;
    const char *what = ""; // names the owner in error messages ("akaze", "ochip_dense_link", ...)
    std::vector<std::pair<void *, size_t>> held;

    dev_blocks() = default;
    dev_blocks(ochip_ctx *c, const char *w) : ctx(c), what(w) {}
    dev_blocks(const dev_blocks &) = delete;
    dev_blocks &operator=(const dev_blocks &) = delete;

    void *get(size_t bytes); // a block of max(bytes, 16); nullptr after ochip_fail(OCHIP_ENOMEM, ...)
    int upload_bytes(void **dst, const void *src, size_t bytes, copy_mode m);
    // get + copy of n elements; src == nullptr or n == 0: allocate only.  OCHIP_ENOMEM / OCHIP_EHIP on failure
    template <class T> int upload(T **dst, const T *src, size_t n, copy_mode m)
    {
        void *d = nullptr;
        const int rc = upload_bytes(&d, src, n * sizeof(T), m);
        if (rc == OCHIP_OK)
            *dst = (T *)d;
        return rc;
    }
    template <class T> int upload(T **dst, const std::vector<T> &v, copy_mode m)
    {
        return upload(dst, v.data(), v.size(), m);
    }
    template <class T> int alloc(T **dst, size_t n)
    {
        return upload<T>(dst, nullptr, n, copy_mode::enqueue);
    }
    // put everything back now: the caller knows that nothing on the stream can still touch the blocks
    void release();
    bool empty() const
    {
        return held.empty();
    }
};

// Call-scoped blocks.  The normal path waits for the stream where it always did and calls release(); an exit that still
// holds blocks (an early return) waits for ctx->stream here first, so that no block reaches the pool under a running kernel.
struct dev_scratch : dev_blocks
{
    using dev_blocks::dev_blocks;
    ~dev_scratch();
};

// features.hip: the tail of extract_features prepared on the device for B images whose compacted keypoints lie in HBM
// (enqueued on the context's stream, results copied into `out`; the caller waits and releases `mem`)
int feature_lists_enqueue(ochip_ctx *ctx, dev_blocks &mem, uint32_t B, uint32_t max_kp, const float *d_kp6,
                          const unsigned long long *d_desc, const unsigned int *d_counts, uint32_t most, int work_w, int work_h,
                          double scale, double nms_radius, const ochip_feature_lists *out);

// mesh_points.hip: the device cloud of a live ochip_mesh_points object (xyz [n][3]) and its context; false otherwise
bool mesh_points_view(const ochip_mesh_points *m, ochip_ctx **ctx, const double **xyz, uint32_t *n);

// std_sort.hip: libstdc++'s std::sort (comp(a, b) = high half of a > high half of b) on segments of 64-bit records in HBM
int std_sort_enqueue(ochip_ctx *ctx, dev_blocks &mem, unsigned long long *recs, size_t total_len, const unsigned int *seg_begin,
                     const unsigned int *seg_end, uint32_t n_segs, uint32_t max_len, unsigned char *fallback);
} // namespace ochip
