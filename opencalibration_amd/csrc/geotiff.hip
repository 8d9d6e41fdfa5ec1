// The tiles of the tiled DEFLATE GeoTIFFs on the device (the rules: deflate_rules.hpp, the encoder's
// kernel bodies: deflate_kernels.hpp).  A feed copies its rows into the tile row being filled; a complete tile row is one pass
// of these launches on the context's stream:
//   gt_payload     512 x 512 tiles out of the rows: 16-byte loads where the width allows, the horizontal predictor, zeros
//                  beyond the raster; a tile's any-non-zero flag
//   gt_parse       a workgroup per 16 384-byte segment: a lane compares its 64 bytes with the pixel to the left and the pixel
//                  above - compile-time distances 4 and 2 048, aligned 16-byte loads of the row above - into two 64-bit masks,
//                  then parse_segment
//   gt_codes       a wave per block: codes_block
//   (rocPRIM)      exclusive scan of the blocks' bits
//   gt_tile_sizes  a lane a tile: its bits, deflated or stored or left out, its Adler-32 from the 64 partials
//   (rocPRIM)      exclusive scan of the tiles' 16-byte-aligned sizes: where each lies in the pass's output
//   gt_emit        a workgroup per block of a deflated tile that fits the slot: emit_segment into the tile's words
//   gt_stored      the stored form of the tiles that did not shrink
//   gt_finish      78 9C and the Adler-32 of the deflated tiles; offsets and counts for the host
// The layers and cameras rasters (section 4.24) take the same pass with a pixel of 8 or 16 bytes: gt_payload_layered
// interleaves the layer-major rows while it predicts, and the kernels behind it are instantiated per pixel size.
// and two copies to page-locked memory: the offsets and counts, and as many bytes as the pass before suggests.  A pass writes
// into one of OUT_SLOTS output slots with an event each; the host reads a slot when a pass needs it again, at collect or at
// finish - one wait, for the slot's event, and so not for what the caller enqueued on the stream since.
#include "deflate_kernels.hpp"
#include "live_handles.hpp"

#include <deque>
#include <memory>
#include <vector>

namespace
{

using namespace ochip_dfk;

constexpr int OUT_SLOTS = 4;

// skip: the tile is all zero and the writer sparse
__device__ bool skipped(const uint32_t *nz, int sparse, int tile)
{
    return sparse && nz[tile] == 0;
}

__global__ __launch_bounds__(THREADS) void gt_payload(const uint32_t *rows, int64_t w, int is_float, int vec, int tiles, uint8_t *payload,
                                                       uint32_t *nz)
{
    const int tile = blockIdx.y, idx = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    const int r = idx >> 7, q = idx & 127;
    if (tile >= tiles || r >= TILE)
        return;
    const int64_t X0 = (int64_t)tile * TILE + q * 4;
    const uint32_t *src = rows + (size_t)r * (size_t)w;
    uint32_t cur[4] = {0, 0, 0, 0};
    if (vec && X0 + 3 < w)
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + X0);
        cur[0] = v.x, cur[1] = v.y, cur[2] = v.z, cur[3] = v.w;
    }
    else
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
            cur[j] = X0 + j < w ? src[X0 + j] : 0;
    }
    const uint32_t left = q > 0 && X0 - 1 < w ? src[X0 - 1] : 0;
    uint4 o;
    o.x = q == 0 ? cur[0] : predict_word(cur[0], left, is_float != 0);
    o.y = predict_word(cur[1], cur[0], is_float != 0);
    o.z = predict_word(cur[2], cur[1], is_float != 0);
    o.w = predict_word(cur[3], cur[2], is_float != 0);
    *reinterpret_cast<uint4 *>(payload + (size_t)tile * PAYLOAD + (size_t)r * ROW_BYTES + (size_t)q * 16) = o;
    const bool any = (cur[0] | cur[1] | cur[2] | cur[3]) != 0;
    if (__ballot(any) != 0 && (threadIdx.x & 63) == 0)
        atomicOr(&nz[tile], 1u);
}

// The layers and cameras rasters: rows is [L][512][w] samples of U words, layer-major as the layer pass
// leaves them; the payload is [row][col][layer][word].  A lane takes the 4 / U pixels whose samples of one layer are 16 bytes,
// predicts them against the same layer of the pixel before, and stores them interleaved: L stores of 16 bytes.  Every index
// into cur, left and o is a constant once unrolled, so they are registers.
template <int L, int U>
__global__ __launch_bounds__(THREADS) void gt_payload_layered(const uint32_t *rows, int64_t w, int vec, int tiles, uint8_t *payload, uint32_t *nz)
{
    constexpr int PPT = 4 / U, PER_ROW = TILE / PPT, PX = 4 * L * U; // a lane's pixels, the lanes of a tile row, a pixel's bytes
    const int tile = blockIdx.y, idx = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    const int r = idx / PER_ROW, q = idx % PER_ROW;
    if (tile >= tiles || r >= TILE)
        return;
    const int64_t X0 = (int64_t)tile * TILE + q * PPT, row_words = w * U;
    uint32_t cur[L][4], left[L][U];
    uint32_t any = 0;
#pragma unroll
    for (int l = 0; l < L; l++)
    {
        const uint32_t *src = rows + ((size_t)l * TILE + (size_t)r) * (size_t)row_words;
        if (vec && X0 + PPT <= w)
        {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + X0 * U);
            cur[l][0] = v.x, cur[l][1] = v.y, cur[l][2] = v.z, cur[l][3] = v.w;
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 4; j++)
                cur[l][j] = X0 * U + j < row_words ? src[X0 * U + j] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            left[l][u] = q > 0 && X0 - 1 < w ? src[(X0 - 1) * U + u] : 0;
        any |= cur[l][0] | cur[l][1] | cur[l][2] | cur[l][3];
    }
    uint32_t o[4 * L];
#pragma unroll
    for (int p = 0; p < PPT; p++)
#pragma unroll
        for (int l = 0; l < L; l++)
#pragma unroll
            for (int u = 0; u < U; u++)
            {
                const uint32_t c = cur[l][p * U + u], before = p == 0 ? left[l][u] : cur[l][(p - 1) * U + u];
                o[(p * L + l) * U + u] = q == 0 && p == 0 ? c : predict_word(c, before, U == 2);
            }
    uint4 *dst = reinterpret_cast<uint4 *>(payload + (size_t)tile * tile_payload(PX) + (size_t)r * tile_row_bytes(PX) + (size_t)q * 16 * L);
#pragma unroll
    for (int k = 0; k < L; k++)
        dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    if (__ballot(any != 0) != 0 && (threadIdx.x & 63) == 0)
        atomicOr(&nz[tile], 1u);
}

// The kernels below are instantiated per pixel size: PX = 4 (RGBA8, float32, one layer of colours) is the tile of section 4.19
// with its distances 4 and 2 048; 8 and 16 are the layered kinds, with the same code and their own constants.
template <int PX>
__global__ __launch_bounds__(THREADS) void gt_parse(const uint8_t *payload, const uint32_t *nz, int sparse, int blocks, uint16_t *tok,
                                                     uint32_t *counts, uint32_t *seg_adler)
{
    constexpr int PAYLOAD = tile_payload(PX), SEGMENTS = tile_segments(PX), DIST_LEFT = PX, DIST_UP = tile_row_bytes(PX);
    constexpr int W = PX / 4; // a pixel's words: the word to the left is W words back
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= blocks)
        return;
    const int tile = b / SEGMENTS, seg = b % SEGMENTS;
    if (skipped(nz, sparse, tile))
        return;
    const uint8_t *a = payload + (size_t)tile * PAYLOAD;
    // the lane's two masks at the tile's fixed geometry: whole chunks, the row above in aligned 16-byte loads
    const int P0 = seg * SEGMENT + t * CHUNK;
    const bool has_left = P0 >= DIST_LEFT, has_up = P0 >= DIST_UP;
    uint32_t prev[W]; // the last W words seen: the pixel before, once unrolled all in registers
    if constexpr (W == 1)
        prev[0] = has_left ? *reinterpret_cast<const uint32_t *>(a + P0 - DIST_LEFT) : 0;
    else if constexpr (W == 2)
    {
        const uint2 p = has_left ? *reinterpret_cast<const uint2 *>(a + P0 - DIST_LEFT) : make_uint2(0, 0);
        prev[0] = p.x, prev[1] = p.y;
    }
    else
    {
        static_assert(W == 4, "a pixel of 4, 8 or 16 bytes");
        const uint4 p = has_left ? *reinterpret_cast<const uint4 *>(a + P0 - DIST_LEFT) : make_uint4(0, 0, 0, 0);
        prev[0] = p.x, prev[1] = p.y, prev[2] = p.z, prev[3] = p.w;
    }
    uint64_t m_left = 0, m_up = 0;
    uint32_t s1 = 0, s2 = 0;
#pragma unroll
    for (int i = 0; i < CHUNK / 16; i++)
    {
        const uint4 c4 = *reinterpret_cast<const uint4 *>(a + P0 + i * 16);
        uint4 u4 = make_uint4(0, 0, 0, 0);
        if (has_up)
            u4 = *reinterpret_cast<const uint4 *>(a + P0 - DIST_UP + i * 16);
        const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w}, u[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const uint32_t xl = c[k] ^ prev[k % W], xu = c[k] ^ u[k];
#pragma unroll
            for (int y = 0; y < 4; y++)
            {
                const int j = i * 16 + k * 4 + y;
                const uint32_t byte = (c[k] >> (8 * y)) & 255u;
                if (((xl >> (8 * y)) & 255u) == 0)
                    m_left |= 1ull << j;
                if (((xu >> (8 * y)) & 255u) == 0)
                    m_up |= 1ull << j;
                s1 += byte, s2 += (uint32_t)(CHUNK - j) * byte;
            }
            prev[k % W] = c[k];
        }
    }
    if (!has_left) // the tile's first pixel has nothing to its left
        m_left &= ~((1ull << DIST_LEFT) - 1);
    if (!has_up)
        m_up = 0;
    parse_segment(m_left, m_up, s1, s2, CHUNK, a, (uint32_t)(seg * SEGMENT), SEGMENT, DIST_LEFT, DIST_UP, tok + (size_t)tile * PAYLOAD,
                  counts + (size_t)b * NUM_SYMS, seg_adler + 2 * (size_t)b);
}

template <int PX>
__global__ __launch_bounds__(64) void gt_codes(const uint32_t *counts, const uint32_t *nz, int sparse, int blocks, uint32_t *codes,
                                                uint32_t *header, uint32_t *header_bits, uint32_t *block_bits)
{
    constexpr int SEGMENTS = tile_segments(PX);
    const int b = blockIdx.x;
    if (b >= blocks)
        return;
    if (skipped(nz, sparse, b / SEGMENTS))
        return; // block_bits was zeroed
    codes_block(counts + (size_t)b * NUM_SYMS, b % SEGMENTS == SEGMENTS - 1, codes + (size_t)b * NUM_SYMS, header + (size_t)b * HEADER_WORDS,
                header_bits + b, block_bits + b);
}

// state: 0 deflated, 1 stored, 2 left out; count: the stream's bytes; size[tiles] = 0 so that the scan's last output is the total
template <int PX>
__global__ __launch_bounds__(THREADS) void gt_tile_sizes(const unsigned long long *block_off, const uint32_t *seg_adler, const uint32_t *nz,
                                                          int sparse, int tiles, uint32_t *state, uint32_t *count, uint32_t *size,
                                                          uint32_t *adler)
{
    constexpr int PAYLOAD = tile_payload(PX), SEGMENTS = tile_segments(PX), STORED_BYTES = tile_stored_bytes(PX);
    const int i = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (i > tiles)
        return;
    if (i == tiles)
    {
        size[i] = 0;
        return;
    }
    if (skipped(nz, sparse, i))
    {
        state[i] = 2, count[i] = 0, size[i] = 0, adler[i] = 0;
        return;
    }
    uint64_t bytes = 0;
    const bool stored = !takes_deflated(block_off[(size_t)(i + 1) * SEGMENTS] - block_off[(size_t)i * SEGMENTS], PAYLOAD, bytes);
    const uint32_t n = stored ? (uint32_t)STORED_BYTES : (uint32_t)bytes;
    state[i] = stored ? 1 : 0, count[i] = n, size[i] = (n + 15u) & ~15u;
    adler[i] = stream_adler(seg_adler + 2 * (size_t)i * SEGMENTS, PAYLOAD);
}

template <int PX>
__global__ __launch_bounds__(THREADS) void gt_emit(const uint8_t *payload, const uint16_t *tok, const uint32_t *codes, const uint32_t *header,
                                                    const uint32_t *header_bits, const unsigned long long *block_off,
                                                    const unsigned long long *tile_off, const uint32_t *state, const uint32_t *size,
                                                    int blocks, uint8_t *out, unsigned long long out_cap)
{
    constexpr int PAYLOAD = tile_payload(PX), SEGMENTS = tile_segments(PX), DIST_LEFT = PX, DIST_UP = tile_row_bytes(PX);
    const int b = blockIdx.x;
    if (b >= blocks)
        return;
    const int tile = b / SEGMENTS, seg = b % SEGMENTS;
    if (state[tile] != 0 || tile_off[tile] + size[tile] > out_cap)
        return;
    const size_t at = (size_t)tile * PAYLOAD + (size_t)seg * SEGMENT;
    emit_segment(payload + at, tok + at, CHUNK, codes + (size_t)b * NUM_SYMS, header + (size_t)b * HEADER_WORDS, header_bits[b],
                 reinterpret_cast<uint32_t *>(out + tile_off[tile]), size[tile] / 4, 16 + (block_off[b] - block_off[(size_t)tile * SEGMENTS]),
                 DIST_LEFT, DIST_UP);
}

template <int PX>
__global__ __launch_bounds__(THREADS) void gt_stored(const uint8_t *payload, const unsigned long long *tile_off, const uint32_t *state,
                                                      const uint32_t *adler, int tiles, uint8_t *out, unsigned long long out_cap)
{
    constexpr int PAYLOAD = tile_payload(PX), TILE_SLOT = tile_slot(PX);
    const int tile = blockIdx.y;
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (tile >= tiles || state[tile] != 1 || i >= (uint32_t)TILE_SLOT / 4 || tile_off[tile] + TILE_SLOT > out_cap)
        return;
    reinterpret_cast<uint32_t *>(out + tile_off[tile])[i] = stored_word(i, payload + (size_t)tile * PAYLOAD, PAYLOAD, adler[tile]);
}

// info: [0, tiles] the tiles' offsets in the slot and the total, [tiles + 1, 2 tiles + 1) their byte counts
__global__ __launch_bounds__(THREADS) void gt_finish(const unsigned long long *tile_off, const uint32_t *state, const uint32_t *count,
                                                      const uint32_t *adler, int tiles, uint8_t *out, unsigned long long out_cap,
                                                      unsigned long long *info)
{
    const int i = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (i > tiles)
        return;
    info[i] = tile_off[i];
    if (i == tiles)
        return;
    info[tiles + 1 + i] = count[i];
    if (state[i] != 0 || tile_off[i] + count[i] > out_cap || count[i] < 6)
        return;
    uint8_t *p = out + tile_off[i];
    p[0] = 0x78, p[1] = 0x9C;
    for (int k = 0; k < 4; k++)
        p[count[i] - 4 + k] = (uint8_t)(adler[i] >> (8 * (3 - k)));
}

ochip::live_set<ochip_geotiff> g_live; // the writers that exist

} // namespace

struct ochip_geotiff
{
    ochip_ctx *ctx = nullptr;
    int kind = 0, sparse = 1;
    int layers = 1, unit = 1, px = PIXEL_BYTES; // a pixel: `layers` samples of `unit` 32-bit words, px bytes
    int64_t w = 0, h = 0, tiles_x = 0, next_row = 0;
    bool finished = false;
    ochip::dev_blocks mem; // everything on the device, held until destroy
    uint32_t *rows = nullptr;  // the tile row being filled: [layers][512][w] samples, zeros where nothing was fed
    uint8_t *payload = nullptr; // [tiles_x][tile_payload(px)]
    uint16_t *tok = nullptr;    // [tiles_x][tile_payload(px)]
    uint32_t *nz = nullptr, *state = nullptr, *count = nullptr, *size = nullptr, *adler = nullptr; // [tiles_x (+ 1)]
    uint32_t *counts = nullptr, *codes = nullptr;                                                  // [blocks][316]
    uint32_t *header = nullptr, *header_bits = nullptr, *block_bits = nullptr, *seg_adler = nullptr;
    unsigned long long *block_off = nullptr, *tile_off = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_bytes = 0, slot_cap = 0;
    struct out_slot
    {
        uint8_t *out = nullptr;
        unsigned long long *info = nullptr;             // [2 tiles_x + 2]
        void *pin_info = nullptr, *pin_bytes = nullptr; // page-locked blocks of the context's pool
        size_t pin_bytes_cap = 0;
        hipEvent_t done = nullptr; // recorded behind the pass's copies
        bool pending = false;
        int tiles = 0;
        size_t guess = 0;
    } slot[OUT_SLOTS];
    uint64_t passes = 0, passes_read = 0;
    double bytes_per_tile = 262144;
    std::deque<std::vector<uint8_t>> ready; // the streams read from the slots, in tile order; empty: a tile left out
};

namespace
{

void release_host_side(ochip_geotiff *e)
{
    for (ochip_geotiff::out_slot &o : e->slot)
    {
        if (o.done)
            (void)hipEventDestroy(o.done);
        ochip_host_free(e->ctx, o.pin_info);
        ochip_host_free(e->ctx, o.pin_bytes);
    }
}

// The oldest pending pass's tiles into the host queue: the one wait
int drain_oldest(ochip_geotiff *e)
{
    ochip_ctx *ctx = e->ctx;
    ochip_geotiff::out_slot &o = e->slot[e->passes_read % OUT_SLOTS];
    if (e->passes_read == e->passes || !o.pending)
        return OCHIP_OK;
    o.pending = false, e->passes_read++;
    OCHIP_HIP(ctx, hipEventSynchronize(o.done));
    const unsigned long long *info = static_cast<const unsigned long long *>(o.pin_info);
    const size_t tiles = (size_t)o.tiles, total = (size_t)info[tiles];
    if (total > e->slot_cap)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_geotiff: %zu bytes from %zu tiles, the slot holds %zu", total, tiles, e->slot_cap);
    std::vector<uint8_t> rest;
    const size_t have = total < o.guess ? total : o.guess;
    if (total > have) // the guess was short: the rest directly
    {
        rest.resize(total - have);
        OCHIP_HIP(ctx, hipMemcpy(rest.data(), o.out + have, total - have, hipMemcpyDeviceToHost));
    }
    const uint8_t *pin = static_cast<const uint8_t *>(o.pin_bytes);
    for (size_t i = 0; i < tiles; i++)
    {
        const size_t at = (size_t)info[i], n = (size_t)info[tiles + 1 + i];
        if (n > (size_t)tile_stored_bytes(e->px) || at + n > total)
            return ochip_fail(ctx, OCHIP_EHIP, "ochip_geotiff: tile %zu of a pass has %zu bytes at %zu of %zu", i, n, at, total);
        std::vector<uint8_t> t(n);
        const size_t from_pin = at >= have ? 0 : (at + n <= have ? n : have - at);
        if (from_pin)
            std::memcpy(t.data(), pin + at, from_pin);
        if (n > from_pin)
            std::memcpy(t.data() + from_pin, rest.data() + (at + from_pin - have), n - from_pin);
        e->ready.push_back(std::move(t));
    }
    if (tiles)
        e->bytes_per_tile = (double)total / (double)tiles;
    return OCHIP_OK;
}

int drain(ochip_geotiff *e)
{
    while (e->passes_read < e->passes)
        OCHIP_TRY(drain_oldest(e));
    return OCHIP_OK;
}

// One pass over the first `tiles` payloads: everything behind gt_payload, enqueued
template <int PX> int encode_pass(ochip_geotiff *e, int tiles)
{
    constexpr int SEGMENTS = tile_segments(PX), TILE_SLOT = tile_slot(PX);
    ochip_ctx *ctx = e->ctx;
    if (tiles < 1 || tiles > e->tiles_x)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff: a pass of %d tiles, at most %lld", tiles, (long long)e->tiles_x);
    hipStream_t st = ctx->stream;
    const int blocks = tiles * SEGMENTS;
    ochip_geotiff::out_slot &o = e->slot[e->passes % OUT_SLOTS];
    while (o.pending) // the slot's last pass has not been read: OUT_SLOTS passes back
        OCHIP_TRY(drain_oldest(e));
    const size_t out_bytes = (size_t)tiles * TILE_SLOT; // <= slot_cap
    OCHIP_HIP(ctx, hipMemsetAsync(o.out, 0, out_bytes, st));
    OCHIP_HIP(ctx, hipMemsetAsync(e->block_bits, 0, ((size_t)blocks + 1) * 4, st));
    hipLaunchKernelGGL(gt_parse<PX>, dim3((uint32_t)blocks), dim3(THREADS), 0, st, e->payload, e->nz, e->sparse, blocks, e->tok, e->counts,
                       e->seg_adler);
    OCHIP_TRY(launched(ctx, "gt_parse"));
    hipLaunchKernelGGL(gt_codes<PX>, dim3((uint32_t)blocks), dim3(64), 0, st, e->counts, e->nz, e->sparse, blocks, e->codes, e->header,
                       e->header_bits, e->block_bits);
    OCHIP_TRY(launched(ctx, "gt_codes"));
    OCHIP_TRY(scan_offsets(ctx, "ochip_geotiff", e->scan_tmp, e->scan_bytes, e->block_bits, e->block_off, (size_t)blocks + 1, st));
    hipLaunchKernelGGL(gt_tile_sizes<PX>, dim3(blocks_of((size_t)tiles + 1)), dim3(THREADS), 0, st, e->block_off, e->seg_adler, e->nz, e->sparse,
                       tiles, e->state, e->count, e->size, e->adler);
    OCHIP_TRY(launched(ctx, "gt_tile_sizes"));
    OCHIP_TRY(scan_offsets(ctx, "ochip_geotiff", e->scan_tmp, e->scan_bytes, e->size, e->tile_off, (size_t)tiles + 1, st));
    hipLaunchKernelGGL(gt_emit<PX>, dim3((uint32_t)blocks), dim3(THREADS), 0, st, e->payload, e->tok, e->codes, e->header, e->header_bits,
                       e->block_off, e->tile_off, e->state, e->size, blocks, o.out, (unsigned long long)out_bytes);
    OCHIP_TRY(launched(ctx, "gt_emit"));
    hipLaunchKernelGGL(gt_stored<PX>, dim3(blocks_of((size_t)TILE_SLOT / 4), (uint32_t)tiles), dim3(THREADS), 0, st, e->payload, e->tile_off,
                       e->state, e->adler, tiles, o.out, (unsigned long long)out_bytes);
    OCHIP_TRY(launched(ctx, "gt_stored"));
    hipLaunchKernelGGL(gt_finish, dim3(blocks_of((size_t)tiles + 1)), dim3(THREADS), 0, st, e->tile_off, e->state, e->count, e->adler, tiles,
                       o.out, (unsigned long long)out_bytes, o.info);
    OCHIP_TRY(launched(ctx, "gt_finish"));
    // the offsets and counts, and the bytes the pass before suggests
    size_t guess = (size_t)(e->bytes_per_tile * 1.25 * (double)tiles) + 4096;
    guess = guess < out_bytes ? guess : out_bytes;
    if (guess > o.pin_bytes_cap)
    {
        ochip_host_free(ctx, o.pin_bytes);
        o.pin_bytes = nullptr, o.pin_bytes_cap = 0;
        const size_t room = guess + guess / 4 < e->slot_cap ? guess + guess / 4 : e->slot_cap;
        OCHIP_TRY(ochip_host_alloc(ctx, room, &o.pin_bytes));
        o.pin_bytes_cap = room;
    }
    OCHIP_HIP(ctx, hipMemcpyAsync(o.pin_info, o.info, (2 * (size_t)tiles + 2) * 8, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, hipMemcpyAsync(o.pin_bytes, o.out, guess, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, hipEventRecord(o.done, st));
    o.pending = true, o.tiles = tiles, o.guess = guess;
    e->passes++;
    return OCHIP_OK;
}

int encode_payloads(ochip_geotiff *e, int tiles)
{
    return e->px == 4 ? encode_pass<4>(e, tiles) : e->px == 8 ? encode_pass<8>(e, tiles) : encode_pass<16>(e, tiles);
}

// The payloads of the complete tile row in e->rows, enqueued
int launch_payload(ochip_geotiff *e, int tiles)
{
    ochip_ctx *ctx = e->ctx;
    hipStream_t st = ctx->stream;
    const int vec = (e->w * e->unit) % 4 == 0 && (uintptr_t)e->rows % 16 == 0;
    if (e->layers == 1 && e->unit == 1) // one layer of colours is the RGBA8 tile
    {
        hipLaunchKernelGGL(gt_payload, dim3((uint32_t)(TILE * 128 / THREADS), (uint32_t)tiles), dim3(THREADS), 0, st, e->rows, e->w,
                           e->kind == OCHIP_GEOTIFF_FLOAT32 ? 1 : 0, vec, tiles, e->payload, e->nz);
        return launched(ctx, "gt_payload");
    }
    const dim3 grid((uint32_t)(TILE * (TILE * e->unit / 4) / THREADS), (uint32_t)tiles);
    if (e->kind == OCHIP_GEOTIFF_LAYERS8)
        hipLaunchKernelGGL((gt_payload_layered<2, 1>), grid, dim3(THREADS), 0, st, e->rows, e->w, vec, tiles, e->payload, e->nz);
    else if (e->layers == 1)
        hipLaunchKernelGGL((gt_payload_layered<1, 2>), grid, dim3(THREADS), 0, st, e->rows, e->w, vec, tiles, e->payload, e->nz);
    else
        hipLaunchKernelGGL((gt_payload_layered<2, 2>), grid, dim3(THREADS), 0, st, e->rows, e->w, vec, tiles, e->payload, e->nz);
    return launched(ctx, "gt_payload_layered");
}

int refuse_feed(ochip_geotiff *e, int64_t row0, int64_t rows)
{
    ochip_ctx *ctx = e->ctx;
    if (e->finished)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_geotiff_feed: rows %lld .. %lld after finish", (long long)row0, (long long)(row0 + rows));
    if (rows < 0 || row0 != e->next_row)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_feed: rows %lld .. %lld where row %lld is next (%s)", (long long)row0,
                          (long long)(row0 + rows), (long long)e->next_row, row0 > e->next_row ? "a gap" : "an overlap");
    if (row0 + rows > e->h)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_feed: rows %lld .. %lld beyond the raster's %lld", (long long)row0,
                          (long long)(row0 + rows), (long long)e->h);
    return OCHIP_OK;
}

// A writer of a checked kind, layer count and size: every buffer from the pixel's bytes
int create(ochip_ctx *ctx, int kind, int layers, int64_t width, int64_t height, int sparse, ochip_geotiff **out)
{
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<ochip_geotiff> e(new ochip_geotiff);
    e->ctx = ctx, e->kind = kind, e->sparse = sparse != 0 && kind != OCHIP_GEOTIFF_FLOAT32, e->w = width, e->h = height;
    e->layers = layers, e->unit = unit_words(kind), e->px = pixel_bytes(kind, layers);
    e->bytes_per_tile *= e->px / PIXEL_BYTES;
    e->tiles_x = (width + TILE - 1) / TILE;
    e->mem.ctx = ctx, e->mem.what = "ochip_geotiff";
    const size_t PAYLOAD = (size_t)tile_payload(e->px), TILE_SLOT = (size_t)tile_slot(e->px); // this writer's, not the 4-byte pixel's
    const size_t tiles = (size_t)e->tiles_x, blocks = tiles * (size_t)tile_segments(e->px);
    const size_t row_words = (size_t)layers * TILE * (size_t)width * (size_t)e->unit;
    e->slot_cap = tiles * TILE_SLOT;
    size_t a = 0, b = 0;
    OCHIP_HIP(ctx, scan_offsets(nullptr, a, nullptr, nullptr, blocks + 1, ctx->stream));
    OCHIP_HIP(ctx, scan_offsets(nullptr, b, nullptr, nullptr, tiles + 1, ctx->stream));
    e->scan_bytes = (a > b ? a : b) + 256;
    int rc = e->mem.alloc(&e->rows, row_words);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->payload, tiles * PAYLOAD);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->tok, tiles * PAYLOAD);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->nz, tiles);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->state, tiles);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->count, tiles);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->size, tiles + 1);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->adler, tiles);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->counts, blocks * NUM_SYMS);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->codes, blocks * NUM_SYMS);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->header, blocks * HEADER_WORDS);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->header_bits, blocks);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->block_bits, blocks + 1);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->seg_adler, blocks * 2);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->block_off, blocks + 1);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->tile_off, tiles + 1);
    if (rc == OCHIP_OK)
        rc = (e->scan_tmp = e->mem.get(e->scan_bytes)) ? OCHIP_OK : OCHIP_ENOMEM;
    for (int k = 0; k < OUT_SLOTS && rc == OCHIP_OK; k++)
    {
        ochip_geotiff::out_slot &o = e->slot[k];
        rc = e->mem.alloc(&o.out, e->slot_cap);
        if (rc == OCHIP_OK)
            rc = e->mem.alloc(&o.info, 2 * tiles + 2);
        if (rc == OCHIP_OK)
            rc = ochip_host_alloc(ctx, (2 * tiles + 2) * 8, &o.pin_info);
        if (rc == OCHIP_OK && hipEventCreateWithFlags(&o.done, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess)
            rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_geotiff_create: hipEventCreateWithFlags failed");
    }
    if (rc == OCHIP_OK && hipMemsetAsync(e->rows, 0, row_words * 4, ctx->stream) != hipSuccess)
        rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_geotiff_create: hipMemsetAsync failed");
    if (rc != OCHIP_OK)
    {
        if (ctx->stream.opened())
            (void)ochip_stream_wait(ctx, ctx->stream);
        release_host_side(e.get());
        e->mem.release();
        return rc;
    }
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

} // namespace

extern "C"
{

int ochip_geotiff_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, int sparse, ochip_geotiff **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_create: out is NULL");
    *out = nullptr;
    if ((kind != OCHIP_GEOTIFF_RGBA8 && kind != OCHIP_GEOTIFF_FLOAT32) || width < 1 || height < 1 || width > OCHIP_GEOTIFF_MAX_SIDE ||
        height > OCHIP_GEOTIFF_MAX_SIDE)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_create: kind 0 (RGBA8) or 1 (float32) and sides of 1 .. %d, not kind %d, %lld x %lld",
                          OCHIP_GEOTIFF_MAX_SIDE, kind, (long long)width, (long long)height);
    return create(ctx, kind, 1, width, height, sparse, out);
}

int ochip_geotiff_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int sparse, ochip_geotiff **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_create_layered: out is NULL");
    *out = nullptr;
    if (!layered_kind(kind) || num_layers < 1 || num_layers > MAX_LAYERS || width < 1 || height < 1 || width > OCHIP_GEOTIFF_MAX_SIDE ||
        height > OCHIP_GEOTIFF_MAX_SIDE)
        return ochip_fail(ctx, OCHIP_EINVAL,
                          "ochip_geotiff_create_layered: kind 2 (layers) or 3 (cameras), 1 .. %d layers and sides of 1 .. %d, not kind %d, "
                          "%d layers, %lld x %lld",
                          MAX_LAYERS, OCHIP_GEOTIFF_MAX_SIDE, kind, num_layers, (long long)width, (long long)height);
    return create(ctx, kind, num_layers, width, height, sparse, out);
}

int ochip_geotiff_feed(ochip_geotiff *e, int64_t row0, int64_t rows, const void *pixels, int on_device)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_geotiff_feed: not a live ochip_geotiff object");
    ochip_ctx *ctx = e->ctx;
    if (!pixels)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_feed: the band is NULL");
    OCHIP_TRY(refuse_feed(e, row0, rows));
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t row_bytes = (size_t)e->w * (size_t)e->unit * 4; // one layer's row
    const uint8_t *band = static_cast<const uint8_t *>(pixels);   // layer-major, as the tile row is
    for (int64_t at = 0; at < rows;)
    {
        const int64_t y = row0 + at, in_tile = y % TILE;
        int64_t n = TILE - in_tile;
        n = n < rows - at ? n : rows - at;
        for (int l = 0; l < e->layers; l++)
            OCHIP_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t *>(e->rows) + ((size_t)l * TILE + (size_t)in_tile) * row_bytes,
                                          band + ((size_t)l * (size_t)rows + (size_t)at) * row_bytes, (size_t)n * row_bytes,
                                          on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        at += n, e->next_row = y + n;
        if (e->next_row % TILE == 0 || e->next_row == e->h)
        {
            const int tiles = (int)e->tiles_x;
            OCHIP_HIP(ctx, hipMemsetAsync(e->nz, 0, (size_t)tiles * 4, st));
            OCHIP_TRY(launch_payload(e, tiles));
            OCHIP_TRY(encode_payloads(e, tiles));
            if (e->next_row < e->h && e->h - e->next_row < TILE) // the last tile row is ragged: zeros below the raster
                OCHIP_HIP(ctx, hipMemsetAsync(e->rows, 0, (size_t)e->layers * TILE * row_bytes, st));
        }
    }
    if (!on_device) // the caller's array may be reused on return
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
    return OCHIP_OK;
}

int ochip_geotiff_payloads(ochip_geotiff *e, const uint8_t *payloads, int64_t n)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_geotiff_payloads: not a live ochip_geotiff object");
    ochip_ctx *ctx = e->ctx;
    if (!payloads || n < 1 || n > e->tiles_x)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_payloads: %lld payloads at %p, 1 .. %lld fit", (long long)n, (const void *)payloads,
                          (long long)e->tiles_x);
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    OCHIP_HIP(ctx, hipMemcpyAsync(e->payload, payloads, (size_t)n * (size_t)tile_payload(e->px), hipMemcpyHostToDevice, st));
    OCHIP_HIP(ctx, hipMemsetAsync(e->nz, 1, (size_t)n * 4, st)); // every payload is encoded
    OCHIP_TRY(encode_payloads(e, (int)n));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, st)); // the caller's array may be reused on return
    return OCHIP_OK;
}

int ochip_geotiff_collect(ochip_geotiff *e, uint8_t *buf, uint64_t cap, uint64_t *bytes, uint64_t *counts, uint64_t max_tiles, uint64_t *tiles)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_geotiff_collect: not a live ochip_geotiff object");
    ochip_ctx *ctx = e->ctx;
    if (!bytes || !tiles)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_collect: no place for the counts");
    OCHIP_TRY(drain(e));
    uint64_t total = 0;
    for (const auto &t : e->ready)
        total += t.size();
    *bytes = total, *tiles = e->ready.size();
    if (!buf && !counts)
        return OCHIP_OK;
    if (!buf || !counts || cap < total || max_tiles < e->ready.size())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_geotiff_collect: room for %llu bytes and %llu tiles, %llu and %zu are ready",
                          (unsigned long long)cap, (unsigned long long)max_tiles, (unsigned long long)total, e->ready.size());
    size_t at = 0, k = 0;
    for (const auto &t : e->ready)
    {
        if (!t.empty())
            std::memcpy(buf + at, t.data(), t.size());
        counts[k++] = t.size(), at += t.size();
    }
    e->ready.clear();
    return OCHIP_OK;
}

int ochip_geotiff_finish(ochip_geotiff *e)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_geotiff_finish: not a live ochip_geotiff object");
    if (e->finished)
        return ochip_fail(e->ctx, OCHIP_ESTATE, "ochip_geotiff_finish: finished already");
    if (e->next_row != e->h)
        return ochip_fail(e->ctx, OCHIP_ESTATE, "ochip_geotiff_finish: rows %lld .. %lld were never fed", (long long)e->next_row, (long long)e->h);
    OCHIP_TRY(drain(e));
    e->finished = true;
    return OCHIP_OK;
}

void ochip_geotiff_destroy(ochip_geotiff *e)
{
    if (!g_live.remove(e))
        return;
    if (e->ctx->stream.opened()) // nothing may still touch the blocks when they go back to the pools
        (void)ochip_stream_wait(e->ctx, e->ctx->stream);
    release_host_side(e);
    e->mem.release();
    delete e;
}

} // extern "C"
