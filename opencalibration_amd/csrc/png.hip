// PNG files of a batch of images on the device (the rules: png_rules.hpp, the DEFLATE encoder's kernel
// bodies: deflate_kernels.hpp).  One call is one set of launches on the context's stream, whatever the images' number and
// sizes: the host lays the images' rows, 16 384-byte segments and output pieces end to end (prefix sums over the batch) and
// every kernel finds its image by bisection, so a thousand thumbnails and one large preview fill the device the same way.
//   png_filter       a wave per row: the five filters' sums by wave reduction, the type byte and the chosen row into the payload
//   png_parse        a workgroup per segment, 64 bytes a lane: the lane's two masks at runtime distances - the byte
//                    bpp to the left out of the lane's own words, the byte a stride above out of aligned words shifted into
//                    place - with a partial last segment, then parse_segment, the walk the GeoTIFF tiles take
//   png_codes        a wave per block: codes_block
//   (rocPRIM)        exclusive scan of the blocks' bits
//   png_sizes        a lane an image: deflated or stored, the Adler-32 from the partials, 78 9C and the Adler-32 of a deflated one
//   (rocPRIM)        exclusive scan of the files' (or their base64's) sizes: where each lies in the output
//   png_emit         a workgroup per block of a deflated image: emit_segment into the image's stream
//   png_stored       the stored form of the images that did not shrink
//   png_crc_pieces   a lane per 4 096 bytes of a stream: its CRC-32
//   png_crc_combine  a workgroup an image: runs of pieces, then pairs of runs, behind "IDAT" by the x^(8 len) mod P rule
//   png_file         signature, IHDR, IDAT's length and type, the stream, its CRC, IEND - into the output, or, for base64,
//                    into a buffer of the files at their bounds
//   png_base64       a lane per 12 input bytes, into the output
// and two copies: the offsets, then as many bytes as they say.  Steps that depend on each other are separate launches.
#include "deflate_kernels.hpp"
#include "live_handles.hpp"
#include "png_rules.hpp"

#include <memory>
#include <vector>

namespace
{

using namespace ochip_png;
using namespace ochip_dfk;

constexpr uint32_t B64_UNIT = 3072; // input bytes a workgroup of png_base64 turns into 4 096 characters
static_assert(CRC_PIECE == THREADS * 16, "png_file moves a piece as 16 bytes a lane");
static_assert(B64_UNIT == THREADS * 12, "png_base64 takes 4 groups of 3 bytes a lane");

// What the kernels know of an image.  Offsets into the batch's buffers; pay_off is a multiple of 64 and the payload's room
// F rounded up to 64, z_off a multiple of 16 and the stream's room S rounded up to 16.
struct img_desc
{
    const uint8_t *pix;
    unsigned long long pay_off, z_off, bound_off;
    uint32_t w, h, c, swap_rb, stride, segs, F, S, room;
};

// the image that owns unit u: base[i] <= u < base[i + 1], base[0] = 0, u < base[n]
__device__ int owner_of(const uint32_t *base, int n, uint32_t u)
{
    int lo = 0, hi = n;
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= u)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(THREADS) void png_filter(const img_desc *descs, const uint32_t *row_base, int n, uint32_t rows, uint8_t *payload)
{
    const uint32_t r = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows)
        return;
    const int i = owner_of(row_base, n, r);
    const uint32_t y = r - row_base[i];
    const uint32_t c = descs[i].c, nb = descs[i].w * c, stride = descs[i].stride;
    const bool swap = descs[i].swap_rb != 0;
    if (y >= descs[i].h)
        return;
    const uint8_t *cur = descs[i].pix + (size_t)y * nb, *above = cur - nb;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (uint32_t x = lane; x < nb; x += 64)
    {
        const uint32_t at = source_index(x, c, swap);
        const int raw = cur[at], a = x >= c ? cur[at - c] : 0, b = y ? above[at] : 0, cc = y && x >= c ? above[at - c] : 0;
        s0 += filter_cost(filter_byte(0, raw, a, b, cc)), s1 += filter_cost(filter_byte(1, raw, a, b, cc));
        s2 += filter_cost(filter_byte(2, raw, a, b, cc)), s3 += filter_cost(filter_byte(3, raw, a, b, cc));
        s4 += filter_cost(filter_byte(4, raw, a, b, cc));
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), s3 = wave_sum(s3), s4 = wave_sum(s4);
    int type = 0;
    uint32_t best = s0;
    if (s1 < best)
        best = s1, type = 1;
    if (s2 < best)
        best = s2, type = 2;
    if (s3 < best)
        best = s3, type = 3;
    if (s4 < best)
        best = s4, type = 4;
    uint8_t *out = payload + descs[i].pay_off + (size_t)y * stride;
    if (lane == 0)
        out[0] = (uint8_t)type;
    for (uint32_t x = lane; x < nb; x += 64)
    {
        const uint32_t at = source_index(x, c, swap);
        const int raw = cur[at], a = x >= c ? cur[at - c] : 0, b = y ? above[at] : 0, cc = y && x >= c ? above[at - c] : 0;
        out[1 + x] = filter_byte(type, raw, a, b, cc);
    }
}

// the lane's count of real bytes in segment [lo, hi)
__device__ __forceinline__ int valid_of(uint32_t lo, uint32_t hi)
{
    const uint32_t P0 = lo + threadIdx.x * CHUNK;
    return P0 >= hi ? 0 : hi - P0 < (uint32_t)CHUNK ? (int)(hi - P0) : CHUNK;
}

__global__ __launch_bounds__(THREADS) void png_parse(const img_desc *descs, const uint32_t *seg_base, int n, uint32_t blocks, const uint8_t *payload,
                                                      uint16_t *tok, uint32_t *counts, uint32_t *seg_adler)
{
    const uint32_t b = blockIdx.x;
    if (b >= blocks)
        return;
    const int img = owner_of(seg_base, n, b);
    const uint32_t F = descs[img].F, dl = descs[img].c, du = descs[img].stride;
    const bool use_up = du <= UP_LIMIT;
    const uint8_t *a = payload + descs[img].pay_off;
    const uint32_t lo = (b - seg_base[img]) * (uint32_t)SEGMENT, hi = F - lo < (uint32_t)SEGMENT ? F : lo + (uint32_t)SEGMENT;
    const uint32_t P0 = lo + threadIdx.x * CHUNK;
    const int valid = valid_of(lo, hi);
    // the lane's two masks at runtime distances, over the `valid` real bytes of its chunk
    uint64_t m_left = 0, m_up = 0;
    uint32_t s1 = 0, s2 = 0;
    if (valid > 0)
    {
        // the lane's 64 bytes: whole 16-byte loads, the payload's room is a multiple of 64
        uint32_t c[16];
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const uint4 v = *reinterpret_cast<const uint4 *>(a + P0 + i * 16);
            c[4 * i] = v.x, c[4 * i + 1] = v.y, c[4 * i + 2] = v.z, c[4 * i + 3] = v.w;
        }
        // bpp to the left: the lane's own words and the word before them, shifted by 4 - bpp bytes
        uint32_t prev = P0 >= 4 ? *reinterpret_cast<const uint32_t *>(a + P0 - 4) : 0;
        const int ls = 8 * (4 - (int)dl);
#pragma unroll
        for (int k = 0; k < 16; k++)
        {
            const uint32_t lw = (uint32_t)((((uint64_t)c[k] << 32) | prev) >> ls);
            m_left |= zero_bytes(c[k] ^ lw, 4 * k);
            prev = c[k];
        }
        if (P0 == 0) // the image's first bytes have nothing to their left
            m_left &= ~((1ull << dl) - 1);
        if (use_up && P0 >= du)
        {
            // a stride above: 17 aligned words from the one that holds byte P0 - stride, shifted into place.  The first lies
            // at or after the payload's start, the last ends at or before P0 + 64.
            const uint32_t o = P0 - du, q = o & 3u;
            const uint32_t *u = reinterpret_cast<const uint32_t *>(a + (o - q));
            uint32_t w0 = u[0];
#pragma unroll
            for (int k = 0; k < 16; k++)
            {
                const uint32_t w1 = (k < 15 || q != 0) ? u[k + 1] : 0;
                const uint32_t uw = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * q));
                m_up |= zero_bytes(c[k] ^ uw, 4 * k);
                w0 = w1;
            }
        }
        else if (use_up && P0 + CHUNK > du)
        {
            // the chunk in which the second row starts: byte by byte
#pragma unroll
            for (int k = 0; k < 16; k++)
#pragma unroll
                for (int y = 0; y < 4; y++)
                {
                    const uint32_t p = P0 + 4 * k + y;
                    if (p >= du && p < hi && a[p - du] == ((c[k] >> (8 * y)) & 255u))
                        m_up |= 1ull << (4 * k + y);
                }
        }
        const uint64_t keep = valid == CHUNK ? ~0ull : (1ull << valid) - 1;
        m_left &= keep, m_up &= keep;
#pragma unroll
        for (int k = 0; k < 16; k++)
#pragma unroll
            for (int y = 0; y < 4; y++)
            {
                const int j = 4 * k + y;
                const uint32_t byte = j < valid ? (c[k] >> (8 * y)) & 255u : 0;
                s1 += byte, s2 += (uint32_t)(valid - j) * byte; // byte = 0 where valid - j would be negative
            }
    }
    parse_segment(m_left, m_up, s1, s2, valid, a, lo, hi - lo, (int)dl, (int)du, tok + descs[img].pay_off, counts + (size_t)b * NUM_SYMS,
                  seg_adler + 2 * (size_t)b);
}

__global__ __launch_bounds__(64) void png_codes(const img_desc *descs, const uint32_t *seg_base, int n, uint32_t blocks, const uint32_t *counts,
                                                 uint32_t *codes, uint32_t *header, uint32_t *header_bits, uint32_t *block_bits)
{
    const uint32_t b = blockIdx.x;
    if (b >= blocks)
        return;
    const int img = owner_of(seg_base, n, b);
    codes_block(counts + (size_t)b * NUM_SYMS, b - seg_base[img] + 1 == descs[img].segs, codes + (size_t)b * NUM_SYMS,
                header + (size_t)b * HEADER_WORDS, header_bits + b, block_bits + b);
}

// state: 0 deflated, 1 stored; zlen: the stream's bytes; osize: the file's bytes, or its base64's; osize[n] = 0 so that the
// scan's last output is the total.  A deflated stream's first two and last four bytes go into the zeroed buffer here.
__global__ __launch_bounds__(THREADS) void png_sizes(const img_desc *descs, const uint32_t *seg_base, int n, const unsigned long long *block_off,
                                                      const uint32_t *seg_adler, int base64, uint32_t *state, uint32_t *zlen, uint32_t *osize,
                                                      uint32_t *adler, uint8_t *zbuf)
{
    const int i = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (i > n)
        return;
    if (i == n)
    {
        osize[i] = 0;
        return;
    }
    const uint32_t F = descs[i].F, s0 = seg_base[i], segs = descs[i].segs;
    uint64_t bytes = 0;
    const bool deflated = takes_deflated(block_off[s0 + segs] - block_off[s0], F, bytes) && bytes <= descs[i].room;
    const uint32_t z = deflated ? (uint32_t)bytes : descs[i].S;
    state[i] = deflated ? 0 : 1, zlen[i] = z;
    const unsigned long long file = (unsigned long long)z + FILE_EXTRA;
    osize[i] = (uint32_t)(base64 ? base64_bytes(file) : file);
    const uint32_t ad = stream_adler(seg_adler + 2 * (size_t)s0, F);
    adler[i] = ad;
    if (deflated)
    {
        uint8_t *p = zbuf + descs[i].z_off;
        p[0] = 0x78, p[1] = 0x9C;
        put_be32(p + z - 4, ad);
    }
}

__global__ __launch_bounds__(THREADS) void png_emit(const img_desc *descs, const uint32_t *seg_base, int n, uint32_t blocks, const uint8_t *payload,
                                                     const uint16_t *tok, const uint32_t *codes, const uint32_t *header, const uint32_t *header_bits,
                                                     const unsigned long long *block_off, const uint32_t *state, const uint32_t *zlen,
                                                     uint8_t *zbuf)
{
    const uint32_t b = blockIdx.x;
    if (b >= blocks)
        return;
    const int img = owner_of(seg_base, n, b);
    if (state[img] != 0)
        return;
    const uint32_t F = descs[img].F;
    const uint32_t lo = (b - seg_base[img]) * (uint32_t)SEGMENT, hi = F - lo < (uint32_t)SEGMENT ? F : lo + (uint32_t)SEGMENT;
    // the words in front of the Adler-32's: the room is the stored form's, a deflated stream is shorter
    const uint32_t cap = (zlen[img] + 3) / 4 < descs[img].room / 4 ? (zlen[img] + 3) / 4 : descs[img].room / 4;
    emit_segment(payload + descs[img].pay_off + lo, tok + descs[img].pay_off + lo, valid_of(lo, hi), codes + (size_t)b * NUM_SYMS,
                 header + (size_t)b * HEADER_WORDS, header_bits[b], reinterpret_cast<uint32_t *>(zbuf + descs[img].z_off), cap,
                 16 + (block_off[b] - block_off[seg_base[img]]), (int)descs[img].c, (int)descs[img].stride);
}

// a workgroup per segment of a stored image: 4 096 words of its stream's room, the last segment's workgroup the rest as well
__global__ __launch_bounds__(THREADS) void png_stored(const img_desc *descs, const uint32_t *seg_base, int n, uint32_t blocks, const uint8_t *payload,
                                                       const uint32_t *state, const uint32_t *adler, uint8_t *zbuf)
{
    const uint32_t b = blockIdx.x;
    if (b >= blocks)
        return;
    const int img = owner_of(seg_base, n, b);
    if (state[img] != 1)
        return;
    const uint32_t seg = b - seg_base[img], words = descs[img].room / 4;
    const uint32_t first = seg * (uint32_t)(SEGMENT / 4);
    const uint32_t end = seg + 1 == descs[img].segs ? words : (first + SEGMENT / 4 < words ? first + SEGMENT / 4 : words);
    uint32_t *out = reinterpret_cast<uint32_t *>(zbuf + descs[img].z_off);
    for (uint32_t wd = first + threadIdx.x; wd < end; wd += THREADS)
        out[wd] = stored_word(wd, payload + descs[img].pay_off, descs[img].F, adler[img]);
}

__global__ __launch_bounds__(THREADS) void png_crc_pieces(const img_desc *descs, const uint32_t *piece_base, int n, uint32_t pieces,
                                                           const uint32_t *zlen, const uint8_t *zbuf, uint32_t *piece_crc)
{
    __shared__ uint32_t table[256];
    table[threadIdx.x] = crc_table_entry(threadIdx.x);
    __syncthreads();
    const uint32_t u = blockIdx.x * THREADS + threadIdx.x;
    if (u >= pieces)
        return;
    const int img = owner_of(piece_base, n, u);
    const uint32_t at = (u - piece_base[img]) * CRC_PIECE, z = zlen[img] < descs[img].room ? zlen[img] : descs[img].room;
    const uint32_t len = at >= z ? 0 : z - at < CRC_PIECE ? z - at : CRC_PIECE;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(zbuf + descs[img].z_off + at); // whole words: the room is a multiple of 16
    uint32_t reg = ~0u;
    for (uint32_t k = 0; k < (len + 3) / 4; k++)
    {
        const uint32_t wd = src[k];
#pragma unroll
        for (uint32_t y = 0; y < 4; y++)
            if (4 * k + y < len)
                reg = table[(reg ^ (wd >> (8 * y))) & 255u] ^ (reg >> 8);
    }
    piece_crc[u] = ~reg;
}

// A workgroup an image: a lane combines its run of consecutive pieces, then the lanes' results pairwise in LDS - the
// combination is associative, a run of len bytes carries (CRC, len) - and "IDAT" goes in front.  An image of one piece (a
// thumbnail) costs one combination, a 64 MB stream 64 in a row and 8 levels instead of 16 384 in a row.
__global__ __launch_bounds__(THREADS) void png_crc_combine(const uint32_t *piece_base, int n, const uint32_t *zlen, const uint32_t *piece_crc,
                                                            uint32_t *idat_crc)
{
    __shared__ uint32_t run_crc[THREADS], run_len[THREADS];
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= n)
        return;
    const uint32_t z = zlen[i], have = piece_base[i + 1] - piece_base[i];
    uint32_t used = (z + CRC_PIECE - 1) / CRC_PIECE;
    used = used < have ? used : have;
    const uint32_t per = (used + THREADS - 1) / THREADS, first = (uint32_t)t * per;
    const uint32_t full = crc_x_pow(8ull * CRC_PIECE);
    uint32_t crc = 0, bytes = 0; // the empty run
    for (uint32_t k = first; k < first + per && k < used; k++)
    {
        const uint32_t len = z - k * CRC_PIECE < CRC_PIECE ? z - k * CRC_PIECE : CRC_PIECE;
        crc = crc_combine(crc, piece_crc[piece_base[i] + k], len == CRC_PIECE ? full : crc_x_pow(8ull * len));
        bytes += len;
    }
    run_crc[t] = crc, run_len[t] = bytes;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1)
    {
        if (t % (2 * o) == 0 && run_len[t + o] != 0)
        {
            run_crc[t] = crc_combine(run_crc[t], run_crc[t + o], crc_x_pow(8ull * run_len[t + o]));
            run_len[t] += run_len[t + o];
        }
        __syncthreads();
    }
    if (t == 0)
        idat_crc[i] = crc_combine(idat_type_crc(), run_crc[0], crc_x_pow(8ull * run_len[0]));
}

// where file i starts: in the output at its scanned offset, or - for base64 - in the buffer of the files at its bound's
__device__ unsigned long long file_at(const img_desc *descs, const unsigned long long *out_off, int base64, int i)
{
    return base64 ? descs[i].bound_off : out_off[i];
}

__global__ __launch_bounds__(THREADS) void png_file(const img_desc *descs, const uint32_t *piece_base, int n, uint32_t pieces, const uint32_t *zlen,
                                                     const uint32_t *idat_crc, const uint8_t *zbuf, const unsigned long long *out_off, int base64,
                                                     uint8_t *files, unsigned long long files_cap)
{
    const uint32_t u = blockIdx.x;
    if (u >= pieces)
        return;
    const int img = owner_of(piece_base, n, u);
    const uint32_t k = u - piece_base[img], z = zlen[img];
    const unsigned long long at = file_at(descs, out_off, base64, img);
    if (z > descs[img].room || at + z + FILE_EXTRA > files_cap)
        return;
    uint8_t *f = files + at;
    if (k == 0 && threadIdx.x == 0)
        file_head(descs[img].w, descs[img].h, descs[img].c, z, f);
    if (k == 0 && threadIdx.x == 64)
        file_tail(idat_crc[img], f + IDAT_AT + z);
    const uint32_t o = k * CRC_PIECE + threadIdx.x * 16;
    if (o >= z)
        return;
    const uint4 v = *reinterpret_cast<const uint4 *>(zbuf + descs[img].z_off + o); // inside the room, a multiple of 16
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    uint8_t *dst = f + IDAT_AT + o;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++)
        if (o + j < z)
            dst[j] = (uint8_t)(wd[j / 4] >> (8 * (j % 4)));
}

__global__ __launch_bounds__(THREADS) void png_base64(const img_desc *descs, const uint32_t *b64_base, int n, uint32_t units, const uint32_t *zlen,
                                                       const uint8_t *files, const unsigned long long *out_off, uint8_t *text,
                                                       unsigned long long text_cap)
{
    const uint32_t u = blockIdx.x;
    if (u >= units)
        return;
    const int img = owner_of(b64_base, n, u);
    const unsigned long long bytes = (unsigned long long)zlen[img] + FILE_EXTRA, quads = (bytes + 2) / 3;
    if (zlen[img] > descs[img].room || out_off[img] + 4 * quads > text_cap)
        return;
    const uint8_t *in = files + descs[img].bound_off;
    uint8_t *out = text + out_off[img];
    const unsigned long long q0 = (unsigned long long)(u - b64_base[img]) * (B64_UNIT / 3);
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const unsigned long long q = q0 + (unsigned long long)r * THREADS + threadIdx.x;
        if (q >= quads)
            continue;
        char c4[4];
        base64_quad(in, bytes, q, c4);
        out[4 * q] = (uint8_t)c4[0], out[4 * q + 1] = (uint8_t)c4[1], out[4 * q + 2] = (uint8_t)c4[2], out[4 * q + 3] = (uint8_t)c4[3];
    }
}

ochip::live_set<ochip_png_encoder> g_live; // the encoders that exist

// A device array of the encoder that only grows: a batch that needs more takes a new block a quarter larger
struct grown
{
    void *p = nullptr;
    size_t bytes = 0;
};

} // namespace

struct ochip_png_encoder
{
    ochip_ctx *ctx = nullptr;
    ochip::dev_blocks mem; // everything on the device, held until destroy or until a batch needs more
    // per batch
    grown descs, bases, pixels, payload, tok, zbuf, files, text, counts, codes, header, header_bits, block_bits, seg_adler, block_off, per_image,
        out_off, piece_crc, scan_tmp;
    void *pin_in = nullptr, *pin_tab = nullptr; // page-locked: the images of a host batch packed, the tables
    size_t pin_in_bytes = 0, pin_tab_bytes = 0;
};

namespace
{

int ensure_pinned(ochip_ctx *ctx, void **p, size_t *have, size_t want)
{
    if (want <= *have)
        return OCHIP_OK;
    ochip_host_free(ctx, *p);
    *p = nullptr, *have = 0;
    const size_t room = want + want / 4 + 4096;
    OCHIP_TRY(ochip_host_alloc(ctx, room, p));
    *have = room;
    return OCHIP_OK;
}

size_t round_up(size_t v, size_t to)
{
    return (v + to - 1) / to * to;
}

} // namespace

extern "C"
{

int ochip_png_encoder_create(ochip_ctx *ctx, ochip_png_encoder **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_png_encoder_create: out is NULL");
    std::unique_ptr<ochip_png_encoder> e(new ochip_png_encoder);
    e->ctx = ctx, e->mem.ctx = ctx, e->mem.what = "ochip_png_encoder";
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

int ochip_png_encoder_encode(ochip_png_encoder *e, int64_t n64, const ochip_png_image *images, int on_device, int base64, uint8_t *out,
                             uint64_t out_cap, uint64_t *offsets)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_png_encoder_encode: not a live ochip_png_encoder object");
    ochip_ctx *ctx = e->ctx;
    // ---- everything is checked before anything is enqueued ----
    if (n64 < 0 || n64 > MAX_BATCH)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_png_encoder_encode: a batch of %lld images, 0 .. %d are taken", (long long)n64, MAX_BATCH);
    if ((n64 && !images) || !out || !offsets)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_png_encoder_encode: the images, the output or the offsets are NULL");
    const int n = (int)n64;
    std::vector<img_desc> descs((size_t)n);
    std::vector<uint32_t> bases(4 * ((size_t)n + 1), 0); // rows, segments, pieces, base64 units: [n + 1] each
    uint32_t *row_base = bases.data(), *seg_base = row_base + n + 1, *piece_base = seg_base + n + 1, *b64_base = piece_base + n + 1;
    uint64_t in_bytes = 0, pay_bytes = 0, z_bytes = 0, bound_bytes = 0, need = 0, rows = 0, segs = 0, pieces = 0, units = 0;
    for (int i = 0; i < n; i++)
    {
        const ochip_png_image &m = images[i];
        shape s;
        if (!m.pixels)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_png_encoder_encode: image %d has no pixels", i);
        if (!make_shape(m.width, m.height, m.channels, m.swap_rb != 0, s))
            return ochip_fail(ctx, OCHIP_EINVAL,
                              "ochip_png_encoder_encode: image %d: %d x %d of %d channels; sides of 1 .. 65535, 1, 3 or 4 channels and a payload "
                              "below 2^31 bytes are taken",
                              i, m.width, m.height, m.channels);
        img_desc &d = descs[(size_t)i];
        d.pix = on_device ? static_cast<const uint8_t *>(m.pixels) : nullptr;
        d.pay_off = pay_bytes, d.z_off = z_bytes, d.bound_off = bound_bytes;
        d.w = s.w, d.h = s.h, d.c = s.c, d.swap_rb = s.swap_rb, d.stride = s.stride, d.segs = s.segs, d.F = (uint32_t)s.F, d.S = (uint32_t)s.S;
        d.room = (uint32_t)round_up((size_t)s.S, 16);
        const uint64_t bound = file_bound(s.F);
        row_base[i] = (uint32_t)rows, seg_base[i] = (uint32_t)segs, piece_base[i] = (uint32_t)pieces, b64_base[i] = (uint32_t)units;
        rows += s.h, segs += s.segs, pieces += (s.S + CRC_PIECE - 1) / CRC_PIECE, units += (bound + B64_UNIT - 1) / B64_UNIT;
        in_bytes += round_up((size_t)s.w * s.h * s.c, 16), pay_bytes += round_up((size_t)s.F, 64), z_bytes += d.room;
        bound_bytes += round_up((size_t)bound, 16);
        need += base64 ? base64_bytes(bound) : bound;
    }
    if (out_cap < need)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_png_encoder_encode: room for %llu bytes, the bounds of the %d images add up to %llu",
                          (unsigned long long)out_cap, n, (unsigned long long)need);
    if (rows > 0x7FFFFFFFull * (THREADS / 64) || segs > 0x7FFFFFFFull || pieces > 0x7FFFFFFFull || units > 0x7FFFFFFFull)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_png_encoder_encode: %llu rows and %llu segments in one call are more than a launch takes",
                          (unsigned long long)rows, (unsigned long long)segs);
    offsets[0] = 0;
    if (n == 0)
        return OCHIP_OK;
    row_base[n] = (uint32_t)rows, seg_base[n] = (uint32_t)segs, piece_base[n] = (uint32_t)pieces, b64_base[n] = (uint32_t)units;
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- room: a batch that needs more of anything waits for the stream, hands every block back and takes new ones ----
    const size_t blocks = (size_t)segs;
    size_t scan_a = 0, scan_b = 0;
    OCHIP_HIP(ctx, scan_offsets(nullptr, scan_a, nullptr, nullptr, blocks + 1, st));
    OCHIP_HIP(ctx, scan_offsets(nullptr, scan_b, nullptr, nullptr, (size_t)n + 1, st));
    struct want
    {
        grown *g;
        size_t bytes;
    } wants[] = {
        {&e->descs, descs.size() * sizeof(img_desc)},
        {&e->bases, bases.size() * 4},
        {&e->pixels, on_device ? 16 : (size_t)in_bytes},
        {&e->payload, (size_t)pay_bytes},
        {&e->tok, (size_t)pay_bytes * 2},
        {&e->zbuf, (size_t)z_bytes},
        {&e->files, base64 ? (size_t)bound_bytes : round_up((size_t)need, 16)},
        {&e->text, base64 ? round_up((size_t)need, 16) : 16},
        {&e->counts, blocks * NUM_SYMS * 4},
        {&e->codes, blocks * NUM_SYMS * 4},
        {&e->header, blocks * HEADER_WORDS * 4},
        {&e->header_bits, blocks * 4},
        {&e->block_bits, (blocks + 1) * 4},
        {&e->seg_adler, blocks * 8},
        {&e->block_off, (blocks + 1) * 8},
        {&e->per_image, 5 * ((size_t)n + 1) * 4}, // state, zlen, osize, adler, idat_crc
        {&e->out_off, ((size_t)n + 1) * 8},
        {&e->piece_crc, (size_t)pieces * 4},
        {&e->scan_tmp, (scan_a > scan_b ? scan_a : scan_b) + 256},
    };
    bool grow = false;
    for (const want &w : wants)
        grow = grow || w.bytes > w.g->bytes;
    if (grow)
    {
        if (ctx->stream.opened())
            OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
        e->mem.release();
        for (const want &w : wants)
            w.g->p = nullptr, w.g->bytes = w.bytes > w.g->bytes ? w.bytes + w.bytes / 4 : w.g->bytes;
        for (const want &w : wants)
        {
            w.g->bytes = round_up(w.g->bytes, 256);
            w.g->p = e->mem.get(w.g->bytes);
            if (!w.g->p)
            {
                e->mem.release();
                for (const want &v : wants)
                    v.g->p = nullptr, v.g->bytes = 0;
                return OCHIP_ENOMEM;
            }
        }
    }
    OCHIP_TRY(ensure_pinned(ctx, &e->pin_tab, &e->pin_tab_bytes, descs.size() * sizeof(img_desc) + bases.size() * 4 + ((size_t)n + 2) * 8));
    if (!on_device)
    {
        OCHIP_TRY(ensure_pinned(ctx, &e->pin_in, &e->pin_in_bytes, (size_t)in_bytes));
        size_t at = 0;
        for (int i = 0; i < n; i++)
        {
            const size_t bytes = (size_t)descs[(size_t)i].w * descs[(size_t)i].h * descs[(size_t)i].c;
            std::memcpy(static_cast<uint8_t *>(e->pin_in) + at, images[i].pixels, bytes);
            descs[(size_t)i].pix = static_cast<const uint8_t *>(e->pixels.p) + at;
            at += round_up(bytes, 16);
        }
        OCHIP_HIP(ctx, hipMemcpyAsync(e->pixels.p, e->pin_in, (size_t)in_bytes, hipMemcpyHostToDevice, st));
    }
    uint8_t *tab = static_cast<uint8_t *>(e->pin_tab);
    std::memcpy(tab, descs.data(), descs.size() * sizeof(img_desc));
    std::memcpy(tab + descs.size() * sizeof(img_desc), bases.data(), bases.size() * 4);
    unsigned long long *pin_off = reinterpret_cast<unsigned long long *>(tab + round_up(descs.size() * sizeof(img_desc) + bases.size() * 4, 8));
    OCHIP_HIP(ctx, hipMemcpyAsync(e->descs.p, tab, descs.size() * sizeof(img_desc), hipMemcpyHostToDevice, st));
    OCHIP_HIP(ctx, hipMemcpyAsync(e->bases.p, tab + descs.size() * sizeof(img_desc), bases.size() * 4, hipMemcpyHostToDevice, st));
    const img_desc *d_descs = static_cast<const img_desc *>(e->descs.p);
    const uint32_t *d_rows = static_cast<const uint32_t *>(e->bases.p), *d_segs = d_rows + n + 1, *d_pieces = d_segs + n + 1, *d_units = d_pieces + n + 1;
    uint8_t *payload = static_cast<uint8_t *>(e->payload.p), *zbuf = static_cast<uint8_t *>(e->zbuf.p);
    uint8_t *files = static_cast<uint8_t *>(e->files.p), *text = static_cast<uint8_t *>(e->text.p);
    uint16_t *tok = static_cast<uint16_t *>(e->tok.p);
    uint32_t *counts = static_cast<uint32_t *>(e->counts.p), *codes = static_cast<uint32_t *>(e->codes.p), *header = static_cast<uint32_t *>(e->header.p);
    uint32_t *header_bits = static_cast<uint32_t *>(e->header_bits.p), *block_bits = static_cast<uint32_t *>(e->block_bits.p);
    uint32_t *seg_adler = static_cast<uint32_t *>(e->seg_adler.p), *piece_crc = static_cast<uint32_t *>(e->piece_crc.p);
    uint32_t *state = static_cast<uint32_t *>(e->per_image.p), *zlen = state + n + 1, *osize = zlen + n + 1, *adler = osize + n + 1, *idat_crc = adler + n + 1;
    unsigned long long *block_off = static_cast<unsigned long long *>(e->block_off.p), *out_off = static_cast<unsigned long long *>(e->out_off.p);
    const uint32_t nb = (uint32_t)blocks, np = (uint32_t)pieces;
    // ---- the launches ----
    OCHIP_HIP(ctx, hipMemsetAsync(zbuf, 0, (size_t)z_bytes, st));
    OCHIP_HIP(ctx, hipMemsetAsync(block_bits, 0, (blocks + 1) * 4, st));
    hipLaunchKernelGGL(png_filter, dim3((uint32_t)((rows + THREADS / 64 - 1) / (THREADS / 64))), dim3(THREADS), 0, st, d_descs, d_rows, n, (uint32_t)rows,
                       payload);
    OCHIP_TRY(launched(ctx, "png_filter"));
    hipLaunchKernelGGL(png_parse, dim3(nb), dim3(THREADS), 0, st, d_descs, d_segs, n, nb, payload, tok, counts, seg_adler);
    OCHIP_TRY(launched(ctx, "png_parse"));
    hipLaunchKernelGGL(png_codes, dim3(nb), dim3(64), 0, st, d_descs, d_segs, n, nb, counts, codes, header, header_bits, block_bits);
    OCHIP_TRY(launched(ctx, "png_codes"));
    OCHIP_TRY(scan_offsets(ctx, "ochip_png_encoder_encode", e->scan_tmp.p, e->scan_tmp.bytes, block_bits, block_off, blocks + 1, st));
    hipLaunchKernelGGL(png_sizes, dim3(blocks_of((size_t)n + 1)), dim3(THREADS), 0, st, d_descs, d_segs, n, block_off, seg_adler, base64 ? 1 : 0, state,
                       zlen, osize, adler, zbuf);
    OCHIP_TRY(launched(ctx, "png_sizes"));
    OCHIP_TRY(scan_offsets(ctx, "ochip_png_encoder_encode", e->scan_tmp.p, e->scan_tmp.bytes, osize, out_off, (size_t)n + 1, st));
    hipLaunchKernelGGL(png_emit, dim3(nb), dim3(THREADS), 0, st, d_descs, d_segs, n, nb, payload, tok, codes, header, header_bits, block_off, state, zlen,
                       zbuf);
    OCHIP_TRY(launched(ctx, "png_emit"));
    hipLaunchKernelGGL(png_stored, dim3(nb), dim3(THREADS), 0, st, d_descs, d_segs, n, nb, payload, state, adler, zbuf);
    OCHIP_TRY(launched(ctx, "png_stored"));
    hipLaunchKernelGGL(png_crc_pieces, dim3(blocks_of(pieces)), dim3(THREADS), 0, st, d_descs, d_pieces, n, np, zlen, zbuf, piece_crc);
    OCHIP_TRY(launched(ctx, "png_crc_pieces"));
    hipLaunchKernelGGL(png_crc_combine, dim3((uint32_t)n), dim3(THREADS), 0, st, d_pieces, n, zlen, piece_crc, idat_crc);
    OCHIP_TRY(launched(ctx, "png_crc_combine"));
    hipLaunchKernelGGL(png_file, dim3(np), dim3(THREADS), 0, st, d_descs, d_pieces, n, np, zlen, idat_crc, zbuf, out_off, base64 ? 1 : 0, files,
                       (unsigned long long)(base64 ? bound_bytes : need));
    OCHIP_TRY(launched(ctx, "png_file"));
    if (base64)
    {
        hipLaunchKernelGGL(png_base64, dim3((uint32_t)units), dim3(THREADS), 0, st, d_descs, d_units, n, (uint32_t)units, zlen, files, out_off, text,
                           (unsigned long long)need);
        OCHIP_TRY(launched(ctx, "png_base64"));
    }
    OCHIP_HIP(ctx, hipMemcpyAsync(pin_off, out_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
    const uint64_t total = pin_off[n];
    if (total > need)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_png_encoder_encode: %llu bytes from %d images whose bounds add up to %llu", (unsigned long long)total, n,
                          (unsigned long long)need);
    OCHIP_HIP(ctx, hipMemcpyAsync(out, base64 ? text : files, (size_t)total, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
    for (int i = 0; i <= n; i++)
        offsets[i] = pin_off[i];
    return OCHIP_OK;
}

void ochip_png_encoder_destroy(ochip_png_encoder *e)
{
    if (!g_live.remove(e))
        return;
    if (e->ctx->stream.opened()) // nothing may still touch the blocks when they go back to the pools
        (void)ochip_stream_wait(e->ctx, e->ctx->stream);
    ochip_host_free(e->ctx, e->pin_in);
    ochip_host_free(e->ctx, e->pin_tab);
    e->mem.release();
    delete e;
}

} // extern "C"
