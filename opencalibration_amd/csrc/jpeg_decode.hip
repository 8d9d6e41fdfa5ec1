// Baseline JPEG decoding on the device (the rules: jpeg_decode.hpp).  The host parses the headers of
// a batch of files and uploads their bytes once; every call runs these launches on the context's stream:
//   jd_sync        the self-synchronising entropy decode.  A file's restart intervals (one when it has no DRI) are cut into
//                  subsequences of S bits, a lane each, a workgroup 256 consecutive ones of one file with that file's
//                  Huffman tables in LDS.  A lane walks the symbols that begin in its subsequence from an entry state (bit
//                  position, block within the MCU, zigzag index) and records its exit state and the blocks it finished.  The
//                  first lane of an interval knows its state; every other takes the exit of the lane before it, and (0, 0)
//                  at its boundary while that lane has none.  Rounds repeat inside the workgroup until no exit changes;
//                  the launch repeats until no lane anywhere had a new entry - the one counter the host reads back.
//   (rocPRIM)      exclusive scan of the finished blocks: the block a subsequence starts in
//   jd_write       the same walk from the settled entry states, now storing int16 coefficients (natural order) into their
//                  block and setting the file's status where the stream is not a JPEG's
//   jd_dc_sums, jd_dc_chunks, jd_dc_apply   DC differences to DC values: sums per chunk of 64 MCUs and component, a walk
//                  over a file's chunks, the chunk's walk again; a restart interval's first MCU starts from 0
//   jd_idct        dequantise and the islow transform, a block per 8 lanes: columns, LDS, rows; 8-byte stores into the
//                  component planes
//   jd_pixels      a lane a pixel: triangle upsampling of the chroma, colour conversion, EXIF orientation, B G R out
// A wrong entry state decodes garbage by construction: the reader returns zeros past the interval's end, every symbol has
// a defined successor, and only jd_write reports errors.
#include "ctx.hpp"
#include "jpeg_decode.hpp"
#include "live_handles.hpp"

#include <rocprim/device/device_scan.hpp>

#include <memory>

namespace
{

using namespace ochip_jd;

constexpr int THREADS = 256;
constexpr int DC_CHUNK = 64; // MCUs per lane of the DC passes
constexpr uint64_t NO_STATE = ~0ull;

struct file_desc
{
    geometry g;
    uint32_t byte_base;                    // the file's bytes in the batch's buffer
    uint32_t interval_base, interval_count;
    uint32_t sub_base, sub_count;          // its subsequences among the batch's
    uint32_t block_base, block_count;      // its blocks among the batch's
    uint32_t chunk_base, chunk_count;      // its DC chunks
    uint32_t table;                        // its tables
    int32_t orientation;                   // the one to apply
    uint64_t plane_base[3];
    uint64_t out_offset;
};

struct dev_interval
{
    uint32_t byte0, byte1;           // in the file
    uint32_t sub_base;               // in the batch
    uint32_t first_block, block_end; // in the file
};

struct wg_desc
{
    uint32_t file, first_sub, count;
};

struct batch
{
    const uint8_t *bytes;
    const tables *tabs;
    const file_desc *files;
    const dev_interval *intervals;
    const wg_desc *wgs;
    uint64_t *exit_state, *entry_used; // per subsequence
    uint32_t *finished, *first_block;  // per subsequence; the scan's input and output
    int16_t *coef;
    int32_t *dc_chunk; // [chunks][4]: the sums of Y, Cb, Cr since the chunk's last reset, whether it has one
    uint8_t *planes;
    uint8_t *out;
    int32_t *status;    // per file
    uint32_t *counters; // [0] lanes that walked, [1] the most rounds of a workgroup
    uint32_t sub_bits;
};

__device__ void load_tables(const tables *src, tables *lds)
{
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d = reinterpret_cast<uint32_t *>(lds);
    for (int i = threadIdx.x; i < (int)(sizeof(tables) / 4); i += THREADS)
        d[i] = s[i];
}
static_assert(sizeof(tables) % 4 == 0, "copied as words");

// The interval of subsequence `sub` (a batch index) of file f
__device__ const dev_interval &interval_of(const batch &B, const file_desc &f, uint32_t sub)
{
    uint32_t lo = 0, hi = f.interval_count - 1;
    const dev_interval *iv = B.intervals + f.interval_base;
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (iv[mid].sub_base <= sub)
            lo = mid;
        else
            hi = mid - 1;
    }
    return iv[lo];
}

__device__ uint32_t interval_subs(const dev_interval &iv, uint32_t sub_bits)
{
    const uint32_t bits = (iv.byte1 - iv.byte0) * 8u;
    return bits ? (bits + sub_bits - 1) / sub_bits : 1u;
}

// Subsequence k of an interval: [start, end) as bit positions of data bits
__device__ void sub_extent(const bit_reader &r, const dev_interval &iv, uint32_t k, uint32_t sub_bits, uint32_t &start, uint32_t &end)
{
    const uint32_t n = interval_subs(iv, sub_bits);
    start = k == 0 ? iv.byte0 * 8u : r.normalise(iv.byte0 + k * (sub_bits / 8u), iv.byte0);
    end = k + 1 >= n ? iv.byte1 * 8u : r.normalise(iv.byte0 + (k + 1) * (sub_bits / 8u), iv.byte0);
    start = start < iv.byte1 * 8u ? start : iv.byte1 * 8u;
    end = end < iv.byte1 * 8u ? end : iv.byte1 * 8u;
}

__global__ __launch_bounds__(THREADS) void jd_sync(const batch B)
{
    __shared__ tables T;
    __shared__ uint64_t ex[THREADS];
    const wg_desc W = B.wgs[blockIdx.x];
    const file_desc &f = B.files[W.file];
    load_tables(B.tabs + f.table, &T);
    const int t = threadIdx.x;
    const bool active = (uint32_t)t < W.count;
    const uint32_t sub = W.first_sub + (uint32_t)t;
    const geometry g = f.g;
    uint32_t k = 0, start = 0, end = 0, end_bit = 0;
    bit_reader r{B.bytes + f.byte_base, 0};
    uint64_t my_entry = NO_STATE, my_exit = NO_STATE;
    uint32_t my_finished = 0;
    if (active)
    {
        const dev_interval &iv = interval_of(B, f, sub);
        k = sub - iv.sub_base;
        r.end = iv.byte1, end_bit = iv.byte1 * 8u;
        sub_extent(r, iv, k, B.sub_bits, start, end);
        my_entry = B.entry_used[sub], my_exit = B.exit_state[sub], my_finished = B.finished[sub];
    }
    const uint64_t exit_before = my_exit;
    ex[t] = my_exit;
    __syncthreads();
    bool walked = false;
    uint32_t rounds = 0;
    for (;;)
    {
        int changed = 0;
        if (active)
        {
            uint64_t entry;
            if (k == 0)
                entry = walk_state{start, 0, 0}.packed();
            else
            {
                entry = t == 0 ? __atomic_load_n(&B.exit_state[sub - 1], __ATOMIC_RELAXED) : ex[t - 1];
                if (entry == NO_STATE)
                    entry = walk_state{start, 0, 0}.packed();
            }
            if (entry != my_entry)
            {
                walk_state s = walk_state::unpacked(entry);
                uint32_t n = 0;
                while (s.pos < end)
                    n += next_symbol(r, T, g, s, end_bit).block_done ? 1u : 0u;
                my_entry = entry, my_finished = n;
                changed = s.packed() != my_exit;
                my_exit = s.packed();
                walked = true;
            }
        }
        __syncthreads();
        ex[t] = my_exit;
        rounds++;
        if (!__syncthreads_or(changed) || rounds > THREADS)
            break;
    }
    if (walked)
    {
        B.entry_used[sub] = my_entry, B.finished[sub] = my_finished;
        __atomic_store_n(&B.exit_state[sub], my_exit, __ATOMIC_RELAXED);
        if (my_exit != exit_before)
            atomicAdd(&B.counters[0], 1u);
    }
    if (t == 0)
        atomicMax(&B.counters[1], rounds);
}

__global__ __launch_bounds__(THREADS) void jd_write(const batch B)
{
    __shared__ tables T;
    const wg_desc W = B.wgs[blockIdx.x];
    const file_desc &f = B.files[W.file];
    load_tables(B.tabs + f.table, &T);
    __syncthreads();
    const int t = threadIdx.x;
    if ((uint32_t)t >= W.count)
        return;
    const uint32_t sub = W.first_sub + (uint32_t)t;
    const geometry g = f.g;
    const dev_interval &iv = interval_of(B, f, sub);
    const uint32_t k = sub - iv.sub_base, end_bit = iv.byte1 * 8u;
    const bit_reader r{B.bytes + f.byte_base, iv.byte1};
    uint32_t start, end;
    sub_extent(r, iv, k, B.sub_bits, start, end);
    walk_state s = k == 0 ? walk_state{start, 0, 0} : walk_state::unpacked(B.exit_state[sub - 1]);
    // the block this subsequence starts in: the blocks finished since the interval's first subsequence
    uint32_t cur = iv.first_block + (B.first_block[sub] - B.first_block[iv.sub_base]);
    bool bad = false;
    int16_t *coef = B.coef + (size_t)f.block_base * 64;
    while (s.pos < end && cur < iv.block_end)
    {
        const symbol y = next_symbol(r, T, g, s, end_bit);
        bad |= y.bad;
        if (y.zz >= 0 && y.zz < 64)
            coef[(size_t)cur * 64 + (y.zz ? (int)T.zz[y.zz] : 0)] = (int16_t)y.value;
        if (y.block_done)
            cur++;
    }
    // the interval's blocks did not come out; what follows the last block is not read, on either route
    if (k + 1 == interval_subs(iv, B.sub_bits) && cur < iv.block_end)
        bad = true;
    if (bad)
        B.status[W.file] = CORRUPT;
}

// MCU m of a file starts a restart interval
__device__ bool resets(const geometry &g, uint32_t m)
{
    return g.ri > 0 && m % (uint32_t)g.ri == 0;
}

// APPLY false: the sums of chunk c's DC differences since its last reset; true: the differences become values
template <bool APPLY> __device__ void dc_walk(const batch &B, const file_desc &f, uint32_t c)
{
    const geometry g = f.g;
    const uint32_t mcus = (uint32_t)g.mw * (uint32_t)g.mh, m0 = c * DC_CHUNK, m1 = m0 + DC_CHUNK < mcus ? m0 + DC_CHUNK : mcus;
    int32_t *chunk = B.dc_chunk + (size_t)(f.chunk_base + c) * 4;
    int32_t pred[3] = {0, 0, 0};
    int32_t reset = 0;
    if (APPLY)
        pred[0] = chunk[0], pred[1] = chunk[1], pred[2] = chunk[2];
    int16_t *coef = B.coef + (size_t)f.block_base * 64;
    for (uint32_t m = m0; m < m1; m++)
    {
        if (resets(g, m))
            pred[0] = pred[1] = pred[2] = 0, reset = 1;
        for (int j = 0; j < g.bpm; j++)
        {
            int16_t *dc = coef + ((size_t)m * (size_t)g.bpm + (size_t)j) * 64;
            const int comp = component_of_block(g, j);
            pred[comp] += *dc;
            if (APPLY)
                *dc = (int16_t)pred[comp];
        }
    }
    if (!APPLY)
        chunk[0] = pred[0], chunk[1] = pred[1], chunk[2] = pred[2], chunk[3] = reset;
}

template <bool APPLY> __global__ __launch_bounds__(THREADS) void jd_dc(const batch B)
{
    const file_desc &f = B.files[blockIdx.y];
    const uint32_t c = blockIdx.x * THREADS + threadIdx.x;
    if (c < f.chunk_count)
        dc_walk<APPLY>(B, f, c);
}

// A lane a file: the chunks' sums become the predictors their first MCU starts from
__global__ __launch_bounds__(THREADS) void jd_dc_chunks(const batch B, uint32_t n_files)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_files)
        return;
    const file_desc &f = B.files[i];
    int32_t run[3] = {0, 0, 0};
    for (uint32_t c = 0; c < f.chunk_count; c++)
    {
        int32_t *chunk = B.dc_chunk + (size_t)(f.chunk_base + c) * 4;
        for (int k = 0; k < 3; k++)
        {
            const int32_t sum = chunk[k];
            chunk[k] = run[k];
            run[k] = chunk[3] ? sum : run[k] + sum;
        }
    }
}

__global__ __launch_bounds__(THREADS) void jd_idct(const batch B)
{
    __shared__ int ws[THREADS / 8][72]; // a block's rows 9 apart
    const file_desc &f = B.files[blockIdx.y];
    const int t = threadIdx.x, l8 = t & 7, lb = t >> 3;
    const uint32_t n = blockIdx.x * (THREADS / 8) + (uint32_t)lb;
    const bool active = n < f.block_count;
    const geometry g = f.g;
    int comp = 0, bx = 0, by = 0;
    if (active)
    {
        place_block(g, n, comp, bx, by);
        const int16_t *coef = B.coef + ((size_t)f.block_base + n) * 64;
        const uint16_t *q = B.tabs[f.table].quant[comp];
        int d[8];
#pragma unroll
        for (int r = 0; r < 8; r++)
            d[r] = dequantise(coef[r * 8 + l8], q[r * 8 + l8]);
        idct8<true>(d);
#pragma unroll
        for (int r = 0; r < 8; r++)
            ws[lb][r * 9 + l8] = d[r];
    }
    __syncthreads();
    if (!active)
        return;
    int d[8];
#pragma unroll
    for (int c = 0; c < 8; c++)
        d[c] = ws[lb][l8 * 9 + c];
    idct8<false>(d);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 4; c++)
        lo |= (uint32_t)clamp255(d[c] + 128) << (8 * c), hi |= (uint32_t)clamp255(d[c + 4] + 128) << (8 * c);
    const int stride = comp == 0 ? g.yw() : g.pcw();
    uint8_t *plane = B.planes + f.plane_base[comp];
    *reinterpret_cast<uint2 *>(plane + (size_t)(by * 8 + l8) * (size_t)stride + (size_t)bx * 8) = make_uint2(lo, hi);
}

__global__ __launch_bounds__(THREADS) void jd_pixels(const batch B)
{
    const file_desc &f = B.files[blockIdx.y];
    const geometry g = f.g;
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (B.status[blockIdx.y] != OK || i >= (uint64_t)g.w * (uint64_t)g.h)
        return;
    const int x = (int)(i % (uint64_t)g.w), y = (int)(i / (uint64_t)g.w);
    int ox, oy;
    oriented(f.orientation, g.w, g.h, x, y, ox, oy);
    const int ow = oriented_width(f.orientation, g.w, g.h);
    uint8_t *px = B.out + f.out_offset + ((size_t)oy * (size_t)ow + (size_t)ox) * 3;
    const int Y = B.planes[f.plane_base[0] + (size_t)y * (size_t)g.yw() + (size_t)x];
    if (g.ncomp == 1)
    {
        px[0] = px[1] = px[2] = (uint8_t)Y;
        return;
    }
    uint8_t bgr[3];
    ycc_to_bgr(Y, chroma_at(B.planes + f.plane_base[1], g.pcw(), g, x, y), chroma_at(B.planes + f.plane_base[2], g.pcw(), g, x, y), bgr);
    px[0] = bgr[0], px[1] = bgr[1], px[2] = bgr[2];
}

ochip::live_set<ochip_jpeg_decoder> g_live; // the decoders that exist

uint32_t blocks_of(uint64_t n)
{
    return (uint32_t)((n + THREADS - 1) / THREADS);
}

int launched(ochip_ctx *ctx, const char *what)
{
    return hipGetLastError() == hipSuccess ? OCHIP_OK : ochip_fail(ctx, OCHIP_EHIP, "%s launch failed", what);
}

size_t round16(size_t n)
{
    return (n + 15) / 16 * 16;
}

} // namespace

struct ochip_jpeg_decoder
{
    ochip_ctx *ctx = nullptr;
    uint32_t sub_bits = DEFAULT_SUBSEQUENCE_BITS;
};

namespace
{

// Everything of a call behind the argument checks; mem holds the device blocks
int decode_batch(ochip_jpeg_decoder *D, ochip::dev_blocks &mem, int64_t n, const uint8_t *const *files, const std::vector<parsed> &P,
                 bool apply, void *out, ochip_jpeg_file_info *info, int32_t *rounds)
{
    ochip_ctx *ctx = D->ctx;
    const uint32_t S = D->sub_bits;
    std::vector<file_desc> fd((size_t)n);
    std::vector<dev_interval> ivs;
    std::vector<wg_desc> wgs;
    std::vector<tables> tabs;
    std::vector<uint8_t> bytes;
    uint64_t subs = 0, blocks = 0, chunks = 0, plane_bytes = 0, max_blocks = 0, max_chunks = 0, max_pixels = 0;
    for (int64_t i = 0; i < n; i++)
    {
        file_desc &f = fd[i];
        f = file_desc();
        f.g = P[i].g;
        f.sub_base = (uint32_t)subs, f.block_base = (uint32_t)blocks, f.chunk_base = (uint32_t)chunks;
        f.interval_base = (uint32_t)ivs.size(), f.table = (uint32_t)tabs.size(), f.byte_base = (uint32_t)bytes.size();
        f.orientation = apply ? P[i].g.orientation : 1;
        if (P[i].status != OK)
        {
            f.g.w = f.g.h = 0; // nothing of it runs
            continue;
        }
        const geometry &g = P[i].g;
        // the bytes up to the scan's end: positions stay the file's own
        bytes.insert(bytes.end(), files[i], files[i] + P[i].scan1);
        bytes.resize(round16(bytes.size()));
        tabs.push_back(P[i].t);
        for (size_t k = 0; k < P[i].intervals.size(); k++)
        {
            const interval &v = P[i].intervals[k];
            dev_interval d;
            d.byte0 = v.byte0, d.byte1 = v.byte1, d.sub_base = (uint32_t)subs;
            d.first_block = v.first_mcu * (uint32_t)g.bpm, d.block_end = d.first_block + interval_mcus(P[i], k) * (uint32_t)g.bpm;
            ivs.push_back(d);
            const uint64_t bits = (uint64_t)(v.byte1 - v.byte0) * 8;
            subs += bits ? (bits + S - 1) / S : 1;
        }
        f.interval_count = (uint32_t)P[i].intervals.size();
        f.sub_count = (uint32_t)(subs - f.sub_base);
        for (uint32_t s0 = 0; s0 < f.sub_count; s0 += THREADS)
            wgs.push_back({(uint32_t)i, f.sub_base + s0, f.sub_count - s0 < (uint32_t)THREADS ? f.sub_count - s0 : (uint32_t)THREADS});
        f.block_count = P[i].mcus() * (uint32_t)g.bpm;
        f.chunk_count = (P[i].mcus() + DC_CHUNK - 1) / DC_CHUNK;
        blocks += f.block_count, chunks += f.chunk_count;
        for (int c = 0; c < g.ncomp; c++)
        {
            f.plane_base[c] = plane_bytes;
            plane_bytes += round16(c == 0 ? (size_t)g.yw() * (size_t)g.yh() : (size_t)g.pcw() * (size_t)g.pch());
        }
        f.out_offset = info[i].offset;
        max_blocks = f.block_count > max_blocks ? f.block_count : max_blocks;
        max_chunks = f.chunk_count > max_chunks ? f.chunk_count : max_chunks;
        const uint64_t px = (uint64_t)g.w * (uint64_t)g.h;
        max_pixels = px > max_pixels ? px : max_pixels;
    }
    if (rounds)
        rounds[0] = rounds[1] = 0;
    if (subs == 0)
        return OCHIP_OK;
    if (bytes.size() >= (1ull << 32) || subs >= (1ull << 31) || blocks >= (1ull << 31))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_decoder_decode: a batch of %zu bytes and %llu blocks, decode it in parts", bytes.size(),
                          (unsigned long long)blocks);
    hipStream_t st = ctx->stream;
    batch B{};
    B.sub_bits = S, B.out = static_cast<uint8_t *>(out);
    uint8_t *d_bytes = nullptr;
    tables *d_tabs = nullptr;
    file_desc *d_files = nullptr;
    dev_interval *d_ivs = nullptr;
    wg_desc *d_wgs = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_bytes = 0;
    OCHIP_TRY(mem.upload(&d_bytes, bytes, ochip::copy_mode::blocking));
    OCHIP_TRY(mem.upload(&d_tabs, tabs, ochip::copy_mode::blocking));
    OCHIP_TRY(mem.upload(&d_files, fd, ochip::copy_mode::blocking));
    OCHIP_TRY(mem.upload(&d_ivs, ivs, ochip::copy_mode::blocking));
    OCHIP_TRY(mem.upload(&d_wgs, wgs, ochip::copy_mode::blocking));
    OCHIP_TRY(mem.alloc(&B.exit_state, subs));
    OCHIP_TRY(mem.alloc(&B.entry_used, subs));
    OCHIP_TRY(mem.alloc(&B.finished, subs));
    OCHIP_TRY(mem.alloc(&B.first_block, subs));
    OCHIP_TRY(mem.alloc(&B.coef, blocks * 64));
    OCHIP_TRY(mem.alloc(&B.dc_chunk, chunks * 4));
    OCHIP_TRY(mem.alloc(&B.planes, plane_bytes));
    OCHIP_TRY(mem.alloc(&B.status, (size_t)n));
    OCHIP_TRY(mem.alloc(&B.counters, 2));
    OCHIP_HIP(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, B.finished, B.first_block, 0u, (size_t)subs, rocprim::plus<uint32_t>(), st));
    scan_tmp = mem.get(scan_bytes + 256);
    if (!scan_tmp)
        return OCHIP_ENOMEM;
    B.bytes = d_bytes, B.tabs = d_tabs, B.files = d_files, B.intervals = d_ivs, B.wgs = d_wgs;
    OCHIP_HIP(ctx, hipMemsetAsync(B.exit_state, 0xFF, subs * 8, st));
    OCHIP_HIP(ctx, hipMemsetAsync(B.entry_used, 0xFF, subs * 8, st));
    OCHIP_HIP(ctx, hipMemsetAsync(B.finished, 0, subs * 4, st));
    OCHIP_HIP(ctx, hipMemsetAsync(B.coef, 0, blocks * 64 * 2, st));
    OCHIP_HIP(ctx, hipMemsetAsync(B.status, 0, (size_t)n * 4, st));
    OCHIP_HIP(ctx, hipMemsetAsync(B.counters, 0, 8, st));
    // the launch repeats until no lane had a new entry: a workgroup's first lane sees what the workgroup before it left
    uint32_t counters[2] = {0, 0}, walked_before = 0, launches = 0;
    for (;;)
    {
        hipLaunchKernelGGL(jd_sync, dim3((uint32_t)wgs.size()), dim3(THREADS), 0, st, B);
        OCHIP_TRY(launched(ctx, "jd_sync"));
        launches++;
        OCHIP_HIP(ctx, hipMemcpyAsync(counters, B.counters, 8, hipMemcpyDeviceToHost, st));
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
        if (counters[0] == walked_before || launches > wgs.size() + 1)
            break;
        walked_before = counters[0];
    }
    if (rounds)
        rounds[0] = (int32_t)launches, rounds[1] = (int32_t)counters[1];
    OCHIP_HIP(ctx, rocprim::exclusive_scan(scan_tmp, scan_bytes, B.finished, B.first_block, 0u, (size_t)subs, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(jd_write, dim3((uint32_t)wgs.size()), dim3(THREADS), 0, st, B);
    OCHIP_TRY(launched(ctx, "jd_write"));
    hipLaunchKernelGGL(jd_dc<false>, dim3(blocks_of(max_chunks), (uint32_t)n), dim3(THREADS), 0, st, B);
    OCHIP_TRY(launched(ctx, "jd_dc_sums"));
    hipLaunchKernelGGL(jd_dc_chunks, dim3(blocks_of((uint64_t)n)), dim3(THREADS), 0, st, B, (uint32_t)n);
    OCHIP_TRY(launched(ctx, "jd_dc_chunks"));
    hipLaunchKernelGGL(jd_dc<true>, dim3(blocks_of(max_chunks), (uint32_t)n), dim3(THREADS), 0, st, B);
    OCHIP_TRY(launched(ctx, "jd_dc_apply"));
    hipLaunchKernelGGL(jd_idct, dim3((uint32_t)((max_blocks + THREADS / 8 - 1) / (THREADS / 8)), (uint32_t)n), dim3(THREADS), 0, st, B);
    OCHIP_TRY(launched(ctx, "jd_idct"));
    hipLaunchKernelGGL(jd_pixels, dim3(blocks_of(max_pixels), (uint32_t)n), dim3(THREADS), 0, st, B);
    OCHIP_TRY(launched(ctx, "jd_pixels"));
    std::vector<int32_t> status((size_t)n);
    OCHIP_HIP(ctx, hipMemcpyAsync(status.data(), B.status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
    for (int64_t i = 0; i < n; i++)
        if (info[i].status == OK)
            info[i].status = status[i];
    return OCHIP_OK;
}

} // namespace

extern "C"
{

int ochip_jpeg_decoder_create(ochip_ctx *ctx, int subsequence_bits, ochip_jpeg_decoder **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_decoder_create: out is NULL");
    *out = nullptr;
    if (subsequence_bits != 0 && (subsequence_bits < MIN_SUBSEQUENCE_BITS || subsequence_bits % 32 != 0 || subsequence_bits > (1 << 20)))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_decoder_create: subsequence_bits %d is neither 0 nor a multiple of 32 in %d .. %d",
                          subsequence_bits, MIN_SUBSEQUENCE_BITS, 1 << 20);
    std::unique_ptr<ochip_jpeg_decoder> d(new ochip_jpeg_decoder);
    d->ctx = ctx;
    d->sub_bits = subsequence_bits ? (uint32_t)subsequence_bits : (uint32_t)DEFAULT_SUBSEQUENCE_BITS;
    g_live.add(d.get());
    *out = d.release();
    return OCHIP_OK;
}

int ochip_jpeg_decoder_decode(ochip_jpeg_decoder *d, int64_t n, const uint8_t *const *files, const uint64_t *sizes, int apply_orientation,
                              void *out, uint64_t out_cap, const uint64_t *offsets, ochip_jpeg_file_info *info, int32_t *rounds)
{
    if (!g_live.has(d))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_jpeg_decoder_decode: not a live ochip_jpeg_decoder object");
    ochip_ctx *ctx = d->ctx;
    std::vector<parsed> P;
    const bool apply = apply_orientation != 0;
    const std::string refusal = plan_batch(n, MAX_BATCH_FILES, files, sizes, apply, out, out_cap, offsets, info, P);
    if (!refusal.empty())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_decoder_decode: %s", refusal.c_str());
    if (n == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    ochip::dev_blocks mem;
    mem.ctx = ctx, mem.what = "ochip_jpeg_decoder";
    const int rc = decode_batch(d, mem, n, files, P, apply, out, info, rounds);
    if (rc != OCHIP_OK && ctx->stream.opened()) // nothing may still touch the blocks when they go back to the pool
        (void)ochip_stream_wait(ctx, ctx->stream);
    mem.release();
    return rc;
}

void ochip_jpeg_decoder_destroy(ochip_jpeg_decoder *d)
{
    if (!g_live.remove(d))
        return;
    delete d;
}

} // extern "C"
