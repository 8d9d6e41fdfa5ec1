// The PNG files of the thumbnails and previews (the reference's cv::imencode(".png") of a node's
// thumbnail, src/io/serialize_MeasurementGraph.cpp:260-267, src/ortho/thumbnail_encode.hpp and the runner's thumb.png).  This
// header is what is PNG in both routes: the row filters and their choice, the payload, the CRC-32 with its combination, the
// chunk layout and base64.  The IDAT body is deflate_rules.hpp's zlib stream of the payload, the candidates the byte bpp to
// the left and - up to a stride of 32 768 - the byte above.  csrc/png.hip runs the rules in kernels, host/png.cpp in loops; the
// header includes nothing of either, so a stand-alone program builds from it.  Any valid file that decodes to the pixels is
// correct; the two routes give the same bytes because every decision is a function of the pixels alone.
#pragma once

#include "deflate_rules.hpp"

namespace ochip_png
{

using namespace ochip_df;

constexpr int MAX_SIDE = 65535, MAX_BATCH = 65535;
constexpr uint32_t UP_LIMIT = 32768; // deflate's window: the byte above is a candidate up to this stride
// signature 8, IHDR 25, IDAT's length, type and CRC 12, IEND 12
constexpr uint64_t FILE_EXTRA = 57, IDAT_AT = 41;
constexpr uint32_t CRC_POLY = 0xEDB88320u, IEND_CRC = 0xAE426082u;
constexpr uint32_t CRC_PIECE = 4096; // the stream's CRC-32 is combined from partials over pieces of this size
constexpr uint64_t STORED_LIMIT = 1ull << 31;

OCHIP_DF_HD bool valid_shape(int64_t w, int64_t h, int64_t c)
{
    return w >= 1 && h >= 1 && w <= MAX_SIDE && h <= MAX_SIDE && (c == 1 || c == 3 || c == 4);
}

OCHIP_DF_HD constexpr uint64_t stride_of(uint64_t w, uint64_t c)
{
    return 1 + w * c;
}

OCHIP_DF_HD constexpr uint64_t payload_bytes(uint64_t w, uint64_t h, uint64_t c)
{
    return h * stride_of(w, c);
}

// The bound every buffer is sized from: the whole file around the stored form.  A deflated stream is taken only where it is
// smaller than the stored one, so no file is larger.
OCHIP_DF_HD constexpr uint64_t file_bound(uint64_t F)
{
    return stored_bytes(F) + FILE_EXTRA;
}

OCHIP_DF_HD constexpr uint64_t base64_bytes(uint64_t n)
{
    return (n + 2) / 3 * 4;
}

static_assert(file_bound(16384) == 16384 + 11 + 57 && file_bound(300 * 301) == 300 * 301 + 2 + 10 + 4 + 57, "the file's bound");
static_assert(FILE_EXTRA == 8 + 25 + 12 + 12 && IDAT_AT == 8 + 25 + 8, "the chunk layout");
static_assert(base64_bytes(1) == 4 && base64_bytes(3) == 4 && base64_bytes(4) == 8, "base64 with padding");
static_assert(payload_bytes(MAX_SIDE, MAX_SIDE, 4) < (1ull << 35), "sizes are 64-bit; a payload from 2^31 on is refused");

// ---- the row filters ----------------------------------------------------------------------------------------------------------
// Byte x of raster row y as the file holds it: channels 0 and 2 exchanged first where swap_rb asks (c >= 3)
OCHIP_DF_HD uint32_t source_index(uint32_t x, uint32_t c, bool swap_rb)
{
    if (!swap_rb || c < 3)
        return x;
    const uint32_t ch = x % c;
    return ch == 0 ? x + 2 : ch == 2 ? x - 2 : x;
}

OCHIP_DF_HD int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// raw: the byte, a: bpp to its left, b: above, c: above left (zeros outside the image)
OCHIP_DF_HD uint8_t filter_byte(int type, int raw, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(raw - pred);
}

OCHIP_DF_HD uint32_t filter_cost(uint8_t v)
{
    return v < 128 ? v : 256u - v;
}

// The filter with the smallest sum, the lowest type on a tie
OCHIP_DF_HD int choose_filter(const uint64_t *sums)
{
    int best = 0;
    for (int t = 1; t < 5; t++)
        if (sums[t] < sums[best])
            best = t;
    return best;
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) ------------------------------------------------------------------------------
OCHIP_DF_HD uint32_t crc_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; k++)
        i = (i & 1) ? (i >> 1) ^ CRC_POLY : i >> 1;
    return i;
}

// one byte into a running register (the register is the CRC's complement: start from ~0, complement at the end)
OCHIP_DF_HD uint32_t crc_step(uint32_t reg, uint8_t byte)
{
    return crc_table_entry((reg ^ byte) & 255u) ^ (reg >> 8);
}

// a(x) b(x) mod P in the reflected representation: bit 31 is x^0
OCHIP_DF_HD uint32_t crc_multiply(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1)
    {
        if (a & m)
            p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

OCHIP_DF_HD uint32_t crc_x_pow(uint64_t bits) // x^bits mod P
{
    uint32_t p = 1u << 31, q = 1u << 30;
    for (; bits; bits >>= 1)
    {
        if (bits & 1)
            p = crc_multiply(q, p);
        q = crc_multiply(q, q);
    }
    return p;
}

// The CRC-32 of piece a followed by piece b from their own CRC-32s; shift = crc_x_pow(8 * bytes of b)
OCHIP_DF_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t shift)
{
    return crc_multiply(shift, crc_a) ^ crc_b;
}

OCHIP_DF_HD void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

// The file's first 41 bytes: signature, IHDR with its CRC, IDAT's length and type
OCHIP_DF_HD void file_head(uint32_t w, uint32_t h, uint32_t c, uint32_t idat_bytes, uint8_t *out)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; i++)
        out[i] = sig[i];
    put_be32(out + 8, 13);
    out[12] = 'I', out[13] = 'H', out[14] = 'D', out[15] = 'R';
    put_be32(out + 16, w), put_be32(out + 20, h);
    out[24] = 8, out[25] = c == 1 ? 0 : c == 3 ? 2 : 6, out[26] = 0, out[27] = 0, out[28] = 0;
    uint32_t reg = ~0u;
    for (int i = 12; i < 29; i++)
        reg = crc_step(reg, out[i]);
    put_be32(out + 29, ~reg);
    put_be32(out + 33, idat_bytes);
    out[37] = 'I', out[38] = 'D', out[39] = 'A', out[40] = 'T';
}

// The file's last 16 bytes: IDAT's CRC and IEND
OCHIP_DF_HD void file_tail(uint32_t idat_crc, uint8_t *out)
{
    put_be32(out, idat_crc);
    put_be32(out + 4, 0);
    out[8] = 'I', out[9] = 'E', out[10] = 'N', out[11] = 'D';
    put_be32(out + 12, IEND_CRC);
}

OCHIP_DF_HD uint32_t idat_type_crc() // CRC-32 of "IDAT", what the stream's pieces are combined behind
{
    uint32_t reg = ~0u;
    reg = crc_step(reg, 'I'), reg = crc_step(reg, 'D'), reg = crc_step(reg, 'A'), reg = crc_step(reg, 'T');
    return ~reg;
}

// ---- base64 (RFC 4648, padded, no line breaks) ---------------------------------------------------------------------------------
OCHIP_DF_HD char base64_char(uint32_t v) // v < 64
{
    return (char)(v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/');
}

// The four characters of input bytes [3 q, 3 q + 3) of n
OCHIP_DF_HD void base64_quad(const uint8_t *in, uint64_t n, uint64_t q, char *out4)
{
    const uint64_t at = 3 * q;
    const uint32_t b0 = in[at], b1 = at + 1 < n ? in[at + 1] : 0, b2 = at + 2 < n ? in[at + 2] : 0;
    out4[0] = base64_char(b0 >> 2);
    out4[1] = base64_char((b0 & 3) << 4 | b1 >> 4);
    out4[2] = at + 1 < n ? base64_char((b1 & 15) << 2 | b2 >> 6) : '=';
    out4[3] = at + 2 < n ? base64_char(b2 & 63) : '=';
}

// An image's sizes, for the host side of both routes
struct shape
{
    uint32_t w = 0, h = 0, c = 0, stride = 0, segs = 0;
    bool swap_rb = false;
    uint64_t F = 0, S = 0;
    // the stream's match candidates: a pixel to the left, and the byte above where deflate's window reaches it
    int dist_left() const
    {
        return (int)c;
    }
    int dist_up() const
    {
        return stride <= UP_LIMIT ? (int)stride : NO_UP;
    }
};

// false: not 1 .. 65 535 squared of 1, 3 or 4 channels, or the stored form would reach 2^31 bytes
inline bool make_shape(int64_t w, int64_t h, int64_t c, bool swap_rb, shape &s)
{
    if (!valid_shape(w, h, c))
        return false;
    const uint64_t F = payload_bytes((uint64_t)w, (uint64_t)h, (uint64_t)c);
    if (stored_bytes(F) >= STORED_LIMIT)
        return false;
    s.w = (uint32_t)w, s.h = (uint32_t)h, s.c = (uint32_t)c, s.stride = (uint32_t)stride_of((uint64_t)w, (uint64_t)c);
    s.segs = (uint32_t)segments_of(F), s.swap_rb = swap_rb, s.F = F, s.S = stored_bytes(F);
    return true;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host route: the same rules in loops ---------------------------------------------------------------------------------
// Row y of the payload: the type byte and the filtered bytes
inline void filter_row(const uint8_t *pixels, const shape &s, uint32_t y, uint8_t *row_out)
{
    const uint32_t n = s.w * s.c, bpp = s.c;
    const uint8_t *cur = pixels + (size_t)y * n, *above = y ? cur - n : nullptr;
    uint64_t sums[5] = {0, 0, 0, 0, 0};
    for (uint32_t x = 0; x < n; x++)
    {
        const int raw = cur[source_index(x, s.c, s.swap_rb)];
        const int a = x >= bpp ? cur[source_index(x - bpp, s.c, s.swap_rb)] : 0;
        const int b = above ? above[source_index(x, s.c, s.swap_rb)] : 0;
        const int c = above && x >= bpp ? above[source_index(x - bpp, s.c, s.swap_rb)] : 0;
        for (int t = 0; t < 5; t++)
            sums[t] += filter_cost(filter_byte(t, raw, a, b, c));
    }
    const int type = choose_filter(sums);
    row_out[0] = (uint8_t)type;
    for (uint32_t x = 0; x < n; x++)
    {
        const int raw = cur[source_index(x, s.c, s.swap_rb)];
        const int a = x >= bpp ? cur[source_index(x - bpp, s.c, s.swap_rb)] : 0;
        const int b = above ? above[source_index(x, s.c, s.swap_rb)] : 0;
        const int c = above && x >= bpp ? above[source_index(x - bpp, s.c, s.swap_rb)] : 0;
        row_out[1 + x] = filter_byte(type, raw, a, b, c);
    }
}

inline const uint32_t *crc_table()
{
    static const struct table
    {
        uint32_t t[256];
        table()
        {
            for (uint32_t i = 0; i < 256; i++)
                t[i] = crc_table_entry(i);
        }
    } T;
    return T.t;
}

inline uint32_t crc32_of(const uint8_t *p, size_t n)
{
    const uint32_t *T = crc_table();
    uint32_t reg = ~0u;
    for (size_t i = 0; i < n; i++)
        reg = T[(reg ^ p[i]) & 255u] ^ (reg >> 8);
    return ~reg;
}

// The CRC-32 of "IDAT" and the stream behind it: partials over pieces of CRC_PIECE bytes, combined
inline uint32_t idat_crc(const uint8_t *stream, uint64_t n)
{
    uint32_t crc = idat_type_crc();
    const uint32_t full = crc_x_pow(8ull * CRC_PIECE);
    for (uint64_t at = 0; at < n; at += CRC_PIECE)
    {
        const uint64_t k = n - at < CRC_PIECE ? n - at : CRC_PIECE;
        crc = crc_combine(crc, crc32_of(stream + at, (size_t)k), k == CRC_PIECE ? full : crc_x_pow(8 * k));
    }
    return crc;
}

// The file of a payload whose segments are marked and coded (deflate_rules.hpp's segment_block); out is cleared first
inline void assemble_file(const uint8_t *a, const shape &s, const uint16_t *marks, const block_out *blocks, std::vector<uint8_t> &out)
{
    bool deflated = false;
    const uint64_t zlen = stream_bytes(blocks, s.F, deflated);
    out.assign((size_t)(zlen + FILE_EXTRA), 0);
    uint8_t *z = out.data() + IDAT_AT;
    write_stream(a, s.F, s.dist_left(), s.dist_up(), marks, blocks, deflated, zlen, z);
    file_head(s.w, s.h, s.c, (uint32_t)zlen, out.data());
    file_tail(idat_crc(z, zlen), z + zlen);
}

// The whole file of one image, serially
inline void encode_image(const uint8_t *pixels, const shape &s, std::vector<uint8_t> &out, std::vector<uint8_t> *payload_out = nullptr)
{
    std::vector<uint8_t> payload((size_t)s.F);
    for (uint32_t y = 0; y < s.h; y++)
        filter_row(pixels, s, y, payload.data() + (size_t)y * s.stride);
    std::vector<uint16_t> marks((size_t)s.F);
    std::vector<block_out> blocks(s.segs);
    for (uint32_t k = 0; k < s.segs; k++)
        segment_block(payload.data(), s.F, k, s.dist_left(), s.dist_up(), marks.data(), blocks[k]);
    assemble_file(payload.data(), s, marks.data(), blocks.data(), out);
    if (payload_out)
        payload_out->swap(payload);
}

inline void base64_encode(const uint8_t *in, uint64_t n, char *out)
{
    for (uint64_t q = 0; q < (n + 2) / 3; q++)
        base64_quad(in, n, q, out + 4 * q);
}
#endif

} // namespace ochip_png
