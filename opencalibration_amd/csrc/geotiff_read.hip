// Reading the tiles of tiled DEFLATE GeoTIFFs on the device (the rules: inflate_rules.hpp).  A call's
// streams go through launches of as many streams as the scratch budget - streams plus payloads, from the context's pool -
// allows; a launch is one copy of its streams and, on the context's stream,
//   gr_inflate    one wavefront a stream, one stream a workgroup.  The symbol walk is wave-uniform: every lane holds the same
//                 bit reader, kept in scalar registers (readfirstlane where a value comes out of LDS) and fed by scalar loads
//                 of the stream's words; the two decode tables lie in LDS; a block's header is read and its tables are built
//                 by lane 0.  The output window is a ring of 64 KiB in LDS - the 32 768 bytes of history, the unflushed
//                 chunk and a match - so a back-reference never reads the kernel's own global stores.  A literal is one
//                 byte by one lane; a match is copied 64 bytes a step, byte i from pos - dist + i % dist: all reads, a
//                 barrier, all writes; a full chunk of 16 KiB goes to the payload in aligned 16-byte stores.
//   gr_check      a workgroup a stream: the payload's Adler-32 from its 16 384-byte segments' partials by the combination
//                 rule of deflate_rules.hpp, against the stream's; the status.  A pass of its own and not partials per
//                 flushed chunk: the sums and their modulo stay off the serial symbol walk and run 256 lanes wide over
//                 bytes that are still in the L2.
//   gr_unpredict  (the tile reader) one wavefront a tile row: each lane sums its run of pixels, a scan across the lanes, the
//                 lane's offset added - bytes per channel in one word, or 32-bit patterns - and the row stored into the
//                 raster at the tile's place, clipped at the raster's edges and cropped to the row window.
#include "ctx.hpp"
#include "inflate_rules.hpp"
#include "live_handles.hpp"

#include <memory>
#include <vector>

namespace
{

using namespace ochip_inf;

constexpr uint32_t RING = 65536, RING_MASK = RING - 1; // the LDS window; every index into it is reduced by the mask
constexpr uint32_t CHUNK = 16384;                      // what one flush stores
constexpr int THREADS = 256;
// gr_inflate's workgroup is one wavefront: its lanes share one bit reader, lane 0 of the workgroup builds the tables, and
// its barriers order the LDS traffic of that one wavefront
constexpr int INFLATE_THREADS = 64;
static_assert(INFLATE_THREADS == 64, "gr_inflate is written for a workgroup of exactly one wavefront");
constexpr uint64_t DEFAULT_BUDGET = (uint64_t)1536 << 20; // 1 024 tiles of 1 MiB and their streams in one launch: every slot of the device stays fed
static_assert(32768 + CHUNK + 258 + 4096 <= RING, "history, the unflushed chunk, a match or a stored step");

// a stream of a call: where it lies in the launch's stream block and its payload in the launch's payload block
struct gr_desc
{
    uint64_t z_off, z_bytes, out_off, expect;
};

// The stream's words through scalar loads: the block is read-only while the kernel runs, so it is addressed as constant
// memory.  base is 4-byte aligned and the block has room for the last word; bytes from n on read as zeros.
struct uniform_source
{
    const uint32_t *base;
    uint64_t n;
    __host__ __device__ uint32_t word(uint64_t i) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t at = 4 * i;
        if (at >= n)
            return 0;
        typedef const __attribute__((address_space(4))) uint32_t *constant_words;
        const uint32_t v = ((constant_words)(uintptr_t)base)[i];
        const uint64_t left = n - at;
        return left >= 4 ? v : v & ((1u << (8 * (uint32_t)left)) - 1);
#else
        return 0;
#endif
    }
};
using reader = bit_reader<uniform_source>;

__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    return (uint64_t)uniform((uint32_t)(v >> 32)) << 32 | uniform((uint32_t)v);
}

// what lane 0 left in the reader, for every lane
__device__ __forceinline__ void make_uniform(reader &in)
{
    in.acc = uniform64(in.acc), in.cnt = uniform(in.cnt), in.next = uniform64(in.next), in.ended = uniform(in.ended ? 1u : 0u) != 0;
}

__global__ __launch_bounds__(INFLATE_THREADS) void gr_inflate(const uint8_t *streams, const gr_desc *desc, int first, int count, uint8_t *payloads,
                                                  int32_t *status, unsigned long long *produced, uint32_t *adler_stored)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING];
    __shared__ huffman lit, dist;
    __shared__ uint8_t lens[MAX_LENS];
    if ((int)blockIdx.x >= count)
        return;
    const int s = first + (int)blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const gr_desc D = desc[s];
    const uint64_t z_off = uniform64(D.z_off), n = uniform64(D.z_bytes), expect64 = uniform64(D.expect);
    const uint32_t expect = (uint32_t)expect64; // at most 2^30
    const uint32_t slot = (uint32_t)slot_of(expect64);
    uint8_t *out = payloads + uniform64(D.out_off);
    if (n == 0) // a sparse tile: nothing to inflate
        return;
    // the stream begins `skip` bytes into its first aligned word
    const uint32_t skip = (uint32_t)(z_off & 3);
    const uint8_t *z = streams + z_off;
    reader in(uniform_source{reinterpret_cast<const uint32_t *>(streams + (z_off - skip)), n + skip}, n + skip);
    in.seek_byte(skip);
    uint32_t have = 0, flushed = 0;
    bool ok = plausible(n, expect64);
    if (ok)
    {
        const uint32_t cmf = in.take(8), flg = in.take(8);
        ok = zlib_header_ok(cmf, flg);
    }
    for (bool last = false; ok && !last;)
    {
        last = in.take(1) != 0;
        const uint32_t type = in.take(2);
        if (in.ended || type == 3)
        {
            ok = false;
            break;
        }
        if (type == 0)
        {
            uint32_t len = 0;
            if (!read_stored_length(in, len) || len > expect - have)
            {
                ok = false;
                break;
            }
            uint64_t at = in.bit_pos() / 8 - skip; // in the stream
            if (at + len > n)
            {
                ok = false;
                break;
            }
            while (len)
            {
                uint32_t step = CHUNK - (have - flushed); // up to the chunk's end, at most 4 096 bytes
                step = step < 4096 ? step : 4096;
                step = step < len ? step : len;
                for (uint32_t j = lane; j < step; j += 64)
                    ring[(have + j) & RING_MASK] = z[at + j];
                have += step, at += step, len -= step;
                if (have - flushed >= CHUNK)
                {
                    __syncthreads();
                    for (uint32_t k = 0; k < CHUNK; k += 1024)
                    {
                        const uint32_t o = flushed + k + lane * 16;
                        const uint4 v = *reinterpret_cast<const uint4 *>(&ring[o & RING_MASK]);
                        if (o + 16 <= slot)
                            *reinterpret_cast<uint4 *>(out + o) = v;
                    }
                    flushed += CHUNK;
                }
            }
            in.seek_byte(at + skip);
            continue;
        }
        // the block's tables: read and built by lane 0, in LDS
        uint32_t built = 0;
        __syncthreads(); // the tables of the block before are no longer read
        if (lane == 0)
            built = read_block_codes(in, type, lit, dist, lens) ? 1u : 0u;
        make_uniform(in);
        built = uniform(built);
        __syncthreads();
        if (!built)
        {
            ok = false;
            break;
        }
        for (;;) // a symbol a turn: every turn adds to `have`, which expect bounds, or ends the block or the stream
        {
            const int sym = decode(in, lit);
            if (sym < 0 || in.ended)
            {
                ok = false;
                break;
            }
            if (sym < 256)
            {
                if (have >= expect)
                {
                    ok = false;
                    break;
                }
                if (lane == 0)
                    ring[have & RING_MASK] = (uint8_t)sym;
                have++;
            }
            else if (sym == 256)
                break;
            else
            {
                if (sym > 285)
                {
                    ok = false;
                    break;
                }
                const uint32_t len = length_base(sym) + in.take(ochip_df::length_extra_bits(sym));
                const int ds = decode(in, dist);
                if (ds < 0 || ds > 29)
                {
                    ok = false;
                    break;
                }
                const uint32_t d = distance_base(ds) + in.take(ochip_df::distance_extra_bits(ds));
                if (in.ended || d > have || len > expect - have)
                {
                    ok = false;
                    break;
                }
                // byte i of the match is byte i % d of the d bytes before it: every source lies before `have`
                const float inv = 1.0f / (float)d;
                __syncthreads(); // what literals and matches wrote is read now
                for (uint32_t base = 0; base < len; base += 64)
                {
                    const uint32_t i = base + lane;
                    // i / d for i < 258 where i >= d: (i + 0.5) / d is at least 0.5 / 257 from a whole number
                    const uint32_t m = i < d ? i : i - d * (uint32_t)(((float)i + 0.5f) * inv);
                    uint8_t b = 0;
                    if (i < len)
                        b = ring[(have - d + m) & RING_MASK];
                    __syncthreads();
                    if (i < len)
                        ring[(have + i) & RING_MASK] = b;
                }
                have += len;
            }
            if (have - flushed >= CHUNK)
            {
                __syncthreads();
                for (uint32_t k = 0; k < CHUNK; k += 1024)
                {
                    const uint32_t o = flushed + k + lane * 16;
                    const uint4 v = *reinterpret_cast<const uint4 *>(&ring[o & RING_MASK]);
                    if (o + 16 <= slot)
                        *reinterpret_cast<uint4 *>(out + o) = v;
                }
                flushed += CHUNK;
            }
        }
    }
    uint32_t adler = 0;
    if (ok)
        ok = have == expect && read_trailer(in, adler);
    if (ok)
    {
        // the last flush: whole 16-byte vectors inside the slot, zeros behind the payload's end
        __syncthreads();
        for (uint32_t o = flushed + lane * 16; o < have; o += 1024)
        {
            uint4 v = *reinterpret_cast<const uint4 *>(&ring[o & RING_MASK]);
            const uint32_t keep = have - o; // >= 1
            if (keep < 16)
            {
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    w[k] = keep >= 4 * k + 4 ? w[k] : keep <= 4 * k ? 0u : w[k] & ((1u << (8 * (keep - 4 * k))) - 1);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (o + 16 <= slot)
                *reinterpret_cast<uint4 *>(out + o) = v;
        }
    }
    if (lane == 0)
    {
        status[s] = ok ? INF_OK : INF_CORRUPT; // OK: but for the Adler-32, which gr_check compares
        produced[s] = have;
        adler_stored[s] = adler;
    }
}

__global__ __launch_bounds__(THREADS) void gr_check(const uint8_t *payloads, const gr_desc *desc, int first, int count,
                                                     const uint32_t *adler_stored, int32_t *status)
{
    __shared__ uint32_t sh1[THREADS], sh2[THREADS];
    if ((int)blockIdx.x >= count)
        return;
    const int s = first + (int)blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (desc[s].z_bytes == 0 || status[s] != INF_OK)
        return;
    const uint32_t F = (uint32_t)desc[s].expect;
    const uint8_t *a = payloads + desc[s].out_off;
    uint32_t a1 = 1, a2 = 0;
    for (uint32_t lo = 0; lo < F; lo += ochip_df::SEGMENT)
    {
        const uint32_t n = F - lo < (uint32_t)ochip_df::SEGMENT ? F - lo : (uint32_t)ochip_df::SEGMENT;
        uint32_t s1 = 0, s2 = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
        {
            const uint32_t j0 = t * 64 + q * 16; // in the segment; the slot is whole 16-byte vectors
            if (j0 >= n)
                continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(a + lo + j0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
            {
                const uint32_t j = j0 + k, byte = j < n ? (w[k >> 2] >> (8 * (k & 3))) & 255u : 0u;
                s1 += byte, s2 += (n - j) * byte;
            }
        }
        sh1[t] = s1, sh2[t] = s2 % ochip_df::ADLER_MOD;
        __syncthreads();
        for (uint32_t o = THREADS / 2; o > 0; o >>= 1)
        {
            if (t < o)
                sh1[t] += sh1[t + o], sh2[t] += sh2[t + o];
            __syncthreads();
        }
        if (t == 0) // the segment on its own: s1 starts at 1, which every byte's s2 counts once
            ochip_df::adler_combine(a1, a2, (1 + sh1[0]) % ochip_df::ADLER_MOD, (n + sh2[0]) % ochip_df::ADLER_MOD, n);
        __syncthreads();
    }
    if (t == 0 && (a2 << 16 | a1) != adler_stored[s])
        status[s] = INF_CORRUPT;
}

// a pixel of the row as one word: 4 samples or a float's pattern, or the 1 or 3 samples there are
__device__ __forceinline__ uint32_t load_pixel(const uint8_t *row, uint32_t p, int bpp)
{
    if (bpp == 4)
        return reinterpret_cast<const uint32_t *>(row)[p];
    if (bpp == 1)
        return row[p];
    return (uint32_t)row[3 * p] | (uint32_t)row[3 * p + 1] << 8 | (uint32_t)row[3 * p + 2] << 16;
}

__device__ __forceinline__ void store_pixel(uint8_t *row, uint32_t p, int bpp, uint32_t v)
{
    if (bpp == 4)
        reinterpret_cast<uint32_t *>(row)[p] = v;
    else if (bpp == 1)
        row[p] = (uint8_t)v;
    else
        row[3 * p] = (uint8_t)v, row[3 * p + 1] = (uint8_t)(v >> 8), row[3 * p + 2] = (uint8_t)(v >> 16);
}

__global__ __launch_bounds__(THREADS) void gr_unpredict(const uint8_t *payloads, const gr_desc *desc, int first, int count, tile_layout L,
                                                         int64_t ty0, int64_t row0, int64_t rows, uint8_t *raster)
{
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * THREADS + threadIdx.x) >> 6;
    const int64_t tile = wave / L.tile_h, r = wave % L.tile_h;
    if (tile >= count)
        return;
    const int64_t g = first + tile, tiles_x = L.tiles_x();
    const int64_t tx = g % tiles_x, y = (ty0 + g / tiles_x) * L.tile_h + r;
    if (y < row0 || y >= row0 + rows || y >= L.height)
        return;
    const int bpp = (int)L.pixel_bytes();
    const int64_t x0 = tx * L.tile_w;
    const uint32_t cols = (uint32_t)(L.width - x0 < L.tile_w ? L.width - x0 : L.tile_w);
    const bool sparse = desc[g].z_bytes == 0, sum = L.predictor == 2, is_float = L.is_float != 0;
    const uint8_t *src = payloads + desc[g].out_off + (size_t)r * (size_t)L.tile_w * (size_t)bpp;
    uint8_t *dst = raster + ((size_t)(y - row0) * (size_t)L.width + (size_t)x0) * (size_t)bpp;
    const uint32_t run = ((uint32_t)L.tile_w + 63) / 64, p0 = lane * run;
    const uint32_t p1 = p0 + run < (uint32_t)L.tile_w ? p0 + run : (uint32_t)L.tile_w;
    uint32_t acc = 0;
    if (sum && !sparse)
    {
        for (uint32_t p = p0; p < p1; p++)
        {
            const uint32_t v = load_pixel(src, p, bpp);
            acc = is_float ? acc + v : add_bytes(acc, v);
        }
        // the lanes' sums scanned: the lane's offset is the sum of the lanes before it
        uint32_t incl = acc;
        for (int o = 1; o < 64; o <<= 1)
        {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
            if ((int)lane >= o)
                incl = is_float ? incl + up : add_bytes(incl, up);
        }
        acc = (uint32_t)__shfl_up((int)incl, 1, 64);
        if (lane == 0)
            acc = 0;
    }
    for (uint32_t p = p0; p < p1 && p < cols; p++)
    {
        uint32_t v = sparse ? 0u : load_pixel(src, p, bpp);
        if (sum)
            v = acc = is_float ? acc + v : add_bytes(acc, v);
        store_pixel(dst, p, bpp, v);
    }
}

// The layers and cameras rasters: a pixel of W = layers x unit 32-bit words, summed at that stride -
// bytes for the colours, whole words for the ids - and placed layer-major, word k of a pixel into plane k / unit.  A wave a
// tile row as above; acc and v are indexed by unrolled constants only.
template <int W>
__global__ __launch_bounds__(THREADS) void gr_unpredict_layered(const uint8_t *payloads, const gr_desc *desc, int first, int count, tile_layout L,
                                                                 int64_t ty0, int64_t row0, int64_t rows, uint32_t *raster)
{
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * THREADS + threadIdx.x) >> 6;
    const int64_t tile = wave / L.tile_h, r = wave % L.tile_h;
    if (tile >= count)
        return;
    const int64_t g = first + tile, tiles_x = L.tiles_x();
    const int64_t tx = g % tiles_x, y = (ty0 + g / tiles_x) * L.tile_h + r;
    if (y < row0 || y >= row0 + rows || y >= L.height)
        return;
    const int64_t x0 = tx * L.tile_w;
    const uint32_t cols = (uint32_t)(L.width - x0 < L.tile_w ? L.width - x0 : L.tile_w);
    const bool sparse = desc[g].z_bytes == 0, sum = L.predictor == 2, words = L.unit == 2;
    const int U = L.unit;
    // a payload's slot and a tile row of W words a pixel, tile_w a multiple of 16, are 16-byte aligned
    const uint32_t *src = reinterpret_cast<const uint32_t *>(payloads + desc[g].out_off) + (size_t)r * (size_t)L.tile_w * W;
    const uint32_t run = ((uint32_t)L.tile_w + 63) / 64, p0 = lane * run;
    const uint32_t p1 = p0 + run < (uint32_t)L.tile_w ? p0 + run : (uint32_t)L.tile_w;
    uint32_t acc[W];
#pragma unroll
    for (int k = 0; k < W; k++)
        acc[k] = 0;
    if (sum && !sparse)
    {
        for (uint32_t p = p0; p < p1; p++)
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                const uint32_t v = src[(size_t)p * W + k];
                acc[k] = words ? acc[k] + v : add_bytes(acc[k], v);
            }
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            uint32_t incl = acc[k];
            for (int o = 1; o < 64; o <<= 1)
            {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
                if ((int)lane >= o)
                    incl = words ? incl + up : add_bytes(incl, up);
            }
            acc[k] = (uint32_t)__shfl_up((int)incl, 1, 64);
            if (lane == 0)
                acc[k] = 0;
        }
    }
    const size_t plane = (size_t)rows * (size_t)L.width * (size_t)U, at = ((size_t)(y - row0) * (size_t)L.width + (size_t)x0) * (size_t)U;
    for (uint32_t p = p0; p < p1 && p < cols; p++)
#pragma unroll
        for (int k = 0; k < W; k++)
        {
            uint32_t v = sparse ? 0u : src[(size_t)p * W + k];
            if (sum)
                v = acc[k] = words ? acc[k] + v : add_bytes(acc[k], v);
            raster[(size_t)(k / U) * plane + at + (size_t)p * U + (k % U)] = v;
        }
}

ochip::live_set<ochip_geotiff_reader> g_live; // the readers that exist

int launched(ochip_ctx *ctx, const char *what)
{
    return hipGetLastError() == hipSuccess ? OCHIP_OK : ochip_fail(ctx, OCHIP_EHIP, "%s launch failed", what);
}

} // namespace

struct ochip_geotiff_reader
{
    ochip_ctx *ctx = nullptr;
    tile_layout L;
    uint64_t budget = DEFAULT_BUDGET;
    int64_t launches = 0;
};

namespace
{

// The streams of a call through the launches the budget allows.  expect: per stream, or nullptr for the reader's tile size.
// With raster (device memory), every launch's payloads are un-predicted and placed.  status, produced: host arrays of n; out:
// nullptr or host memory that takes the payloads, slot by slot.
int run_streams(ochip_geotiff_reader *r, const char *what, int64_t n, const uint8_t *streams, const uint64_t *offsets, const uint64_t *expect,
                uint8_t *out, uint64_t out_cap, int32_t *status, uint64_t *produced, int64_t ty0, int64_t row0, int64_t rows, uint8_t *raster)
{
    ochip_ctx *ctx = r->ctx;
    if (n == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the launches: streams i0 .. i1 whose streams and payload slots fit the budget, at least one
    std::vector<gr_desc> D((size_t)n);
    std::vector<int64_t> cuts{0};
    uint64_t most_z = 0, most_out = 0, z = 0, o = 0;
    for (int64_t i = 0; i < n; i++)
    {
        const uint64_t zb = offsets[i + 1] - offsets[i], e = expect ? expect[i] : r->L.tile_bytes();
        const uint64_t room = zb || expect ? slot_of(e) : 0; // a sparse tile has no payload; every stream of an inflate has a slot
        const uint64_t need = zb + room;
        if (i > cuts.back() && z + o + need > r->budget)
            cuts.push_back(i), z = 0, o = 0;
        D[(size_t)i] = gr_desc{offsets[i] - offsets[cuts.back()], zb, o, e};
        z = offsets[i + 1] - offsets[cuts.back()], o += room;
        most_z = most_z > z ? most_z : z, most_out = most_out > o ? most_out : o;
    }
    cuts.push_back(n);
    ochip::dev_scratch mem(ctx, what);
    uint8_t *d_streams = nullptr, *d_payloads = nullptr;
    gr_desc *d_desc = nullptr;
    int32_t *d_status = nullptr;
    unsigned long long *d_produced = nullptr;
    uint32_t *d_adler = nullptr;
    OCHIP_TRY(mem.alloc(&d_streams, (size_t)most_z + 16)); // room for the last word of the last stream
    OCHIP_TRY(mem.alloc(&d_payloads, (size_t)most_out + 16));
    OCHIP_TRY(mem.upload(&d_desc, D, ochip::copy_mode::enqueue));
    OCHIP_TRY(mem.alloc(&d_status, (size_t)n));
    OCHIP_TRY(mem.alloc(&d_produced, (size_t)n));
    OCHIP_TRY(mem.alloc(&d_adler, (size_t)n));
    OCHIP_HIP(ctx, hipMemsetAsync(d_status, 0, (size_t)n * 4, st)); // a sparse tile is OK with 0 bytes
    OCHIP_HIP(ctx, hipMemsetAsync(d_produced, 0, (size_t)n * 8, st));
    for (size_t c = 0; c + 1 < cuts.size(); c++)
    {
        const int64_t i0 = cuts[c], i1 = cuts[c + 1];
        const uint64_t zb = offsets[i1] - offsets[i0];
        if (zb) // the launch's streams in one copy
            OCHIP_HIP(ctx, hipMemcpyAsync(d_streams, streams + offsets[i0], (size_t)zb, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(gr_inflate, dim3((uint32_t)(i1 - i0)), dim3(INFLATE_THREADS), 0, st, d_streams, d_desc, (int)i0, (int)(i1 - i0), d_payloads, d_status,
                           d_produced, d_adler);
        OCHIP_TRY(launched(ctx, "gr_inflate"));
        hipLaunchKernelGGL(gr_check, dim3((uint32_t)(i1 - i0)), dim3(THREADS), 0, st, d_payloads, d_desc, (int)i0, (int)(i1 - i0), d_adler,
                           d_status);
        OCHIP_TRY(launched(ctx, "gr_check"));
        r->launches++;
        if (raster)
        {
            const int64_t waves = (i1 - i0) * r->L.tile_h;
            const dim3 grid((uint32_t)((waves * 64 + THREADS - 1) / THREADS));
            uint32_t *planes = reinterpret_cast<uint32_t *>(raster);
            const int W = r->L.layers * r->L.unit;
            if (W == 0)
                hipLaunchKernelGGL(gr_unpredict, grid, dim3(THREADS), 0, st, d_payloads, d_desc, (int)i0, (int)(i1 - i0), r->L, ty0, row0, rows,
                                   raster);
            else if (W == 1)
                hipLaunchKernelGGL(gr_unpredict_layered<1>, grid, dim3(THREADS), 0, st, d_payloads, d_desc, (int)i0, (int)(i1 - i0), r->L, ty0,
                                   row0, rows, planes);
            else if (W == 2)
                hipLaunchKernelGGL(gr_unpredict_layered<2>, grid, dim3(THREADS), 0, st, d_payloads, d_desc, (int)i0, (int)(i1 - i0), r->L, ty0,
                                   row0, rows, planes);
            else
                hipLaunchKernelGGL(gr_unpredict_layered<4>, grid, dim3(THREADS), 0, st, d_payloads, d_desc, (int)i0, (int)(i1 - i0), r->L, ty0,
                                   row0, rows, planes);
            OCHIP_TRY(launched(ctx, "gr_unpredict"));
        }
        if (out)
        {
            uint64_t at = 0;
            for (int64_t i = 0; i < i0; i++)
                at += slot_of(D[(size_t)i].expect);
            uint64_t bytes = 0;
            for (int64_t i = i0; i < i1; i++)
                bytes += slot_of(D[(size_t)i].expect);
            bytes = bytes < out_cap - at ? bytes : out_cap - at; // the last payload's slot may end behind out
            if (bytes)
                OCHIP_HIP(ctx, hipMemcpyAsync(out + at, d_payloads, (size_t)bytes, hipMemcpyDeviceToHost, st));
        }
    }
    OCHIP_HIP(ctx, hipMemcpyAsync(status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, hipMemcpyAsync(produced, d_produced, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
    mem.release();
    return OCHIP_OK;
}

} // namespace

extern "C"
{

int ochip_geotiff_reader_create(ochip_ctx *ctx, int samples, int is_float, int64_t width, int64_t height, int tile_w, int tile_h, int predictor,
                                uint64_t scratch_budget, ochip_geotiff_reader **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<ochip_geotiff_reader> r(new ochip_geotiff_reader);
    r->ctx = ctx;
    tile_layout &L = r->L;
    L.samples = samples, L.is_float = is_float != 0, L.tile_w = tile_w, L.tile_h = tile_h, L.predictor = predictor;
    L.width = width, L.height = height;
    if (const char *why = refuse_layout(L))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_create: %s", why);
    r->budget = scratch_budget ? scratch_budget : DEFAULT_BUDGET;
    g_live.add(r.get());
    *out = r.release();
    return OCHIP_OK;
}

int ochip_geotiff_reader_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int tile_w, int tile_h,
                                        int predictor, uint64_t scratch_budget, ochip_geotiff_reader **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_create_layered: out is NULL");
    *out = nullptr;
    std::unique_ptr<ochip_geotiff_reader> r(new ochip_geotiff_reader);
    r->ctx = ctx;
    if (const char *why = layered_layout(r->L, kind, num_layers, width, height, tile_w, tile_h, predictor))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_create_layered: %s", why);
    r->budget = scratch_budget ? scratch_budget : DEFAULT_BUDGET;
    g_live.add(r.get());
    *out = r.release();
    return OCHIP_OK;
}

int ochip_geotiff_reader_inflate(ochip_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets, const uint64_t *expect,
                                 uint8_t *out, uint64_t out_cap, int32_t *status, uint64_t *bytes)
{
    if (!g_live.has(r))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_geotiff_reader_inflate: not a live ochip_geotiff_reader object");
    if (const char *why = refuse_inflate(n, streams, offsets, expect, out, out_cap, status, bytes))
        return ochip_fail(r->ctx, OCHIP_EINVAL, "ochip_geotiff_reader_inflate: %s", why);
    OCHIP_TRY(run_streams(r, "ochip_geotiff_reader_inflate", n, streams, offsets, expect, out, out_cap, status, bytes, 0, 0, 0, nullptr));
    for (int64_t i = 0; i < n; i++)
        if (offsets[i + 1] == offsets[i]) // no stream at all: the kernel left it alone
            status[i] = INF_CORRUPT, bytes[i] = 0;
    return OCHIP_OK;
}

int ochip_geotiff_reader_read(ochip_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets, int64_t row0, int64_t rows,
                              void *raster, int on_device, int64_t *bad_tile)
{
    if (!g_live.has(r))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_geotiff_reader_read: not a live ochip_geotiff_reader object");
    ochip_ctx *ctx = r->ctx;
    const tile_layout &L = r->L;
    if (const char *why = refuse_read(L, n, streams, offsets, row0, rows, raster, bad_tile))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_read: %s", why);
    if (on_device && L.pixel_bytes() == 4 && (uintptr_t)raster % 4 != 0)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_read: a device raster of 4-byte pixels is 4-byte aligned");
    if (on_device && L.layers && (uintptr_t)raster % 4 != 0)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_reader_read: a device raster of layers is 4-byte aligned");
    *bad_tile = -1;
    if (n == 0 || rows == 0)
        return OCHIP_OK;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t raster_bytes = (size_t)rows * (size_t)L.width * (size_t)L.pixel_bytes();
    ochip::dev_scratch mem(ctx, "ochip_geotiff_reader_read");
    uint8_t *d_raster = static_cast<uint8_t *>(raster);
    if (!on_device)
        OCHIP_TRY(mem.alloc(&d_raster, raster_bytes));
    std::vector<int32_t> status((size_t)n);
    std::vector<uint64_t> produced((size_t)n);
    OCHIP_TRY(run_streams(r, "ochip_geotiff_reader_read", n, streams, offsets, nullptr, nullptr, 0, status.data(), produced.data(), row0 / L.tile_h,
                          row0, rows, d_raster));
    for (int64_t i = 0; i < n && *bad_tile < 0; i++)
        if (status[(size_t)i] != INF_OK)
            *bad_tile = i;
    if (!on_device)
    {
        if (*bad_tile < 0)
            OCHIP_HIP(ctx, hipMemcpy(raster, d_raster, raster_bytes, hipMemcpyDeviceToHost));
        mem.release();
    }
    return OCHIP_OK;
}

int64_t ochip_geotiff_reader_launches(ochip_geotiff_reader *r)
{
    return g_live.has(r) ? r->launches : -1;
}

void ochip_geotiff_reader_destroy(ochip_geotiff_reader *r)
{
    if (!g_live.remove(r))
        return;
    delete r;
}

} // extern "C"
