// The PNG files of the thumbnails and previews (the reference's cv::imencode(".png") of a node's
// thumbnail, src/io/serialize_MeasurementGraph.cpp:260-267, src/ortho/thumbnail_encode.hpp and the runner's thumb.png).  This
// header is the rules for both routes: the row filters and their choice, the payload, the match candidates at runtime
// distances, the block coder of deflate_rules.hpp around them, the stored fallback, the CRC-32 with its combination, the chunk
// layout and base64.  csrc/png.hip runs them in kernels, host/png.cpp in loops; it includes nothing of either, so a
// stand-alone program builds from it.  Any valid file that decodes to the pixels is correct; the two routes give the same
// bytes because every decision below is a function of the pixels alone.
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

OCHIP_DF_HD constexpr uint64_t segments_of(uint64_t F)
{
    return (F + SEGMENT - 1) / SEGMENT;
}

// The stored form: 78 9C, ceil(F / 65 535) stored blocks of 5 bytes of header each, the Adler-32
OCHIP_DF_HD constexpr uint64_t stored_bytes(uint64_t F)
{
    return 2 + F + 5 * ((F + STORED_BLOCK - 1) / STORED_BLOCK) + 4;
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

static_assert(stored_bytes(1) == 12 && stored_bytes(65535) == 65535 + 11 && stored_bytes(65536) == 65536 + 16, "the stored form");
static_assert(file_bound(16384) == 16384 + 11 + 57 && file_bound(300 * 301) == 300 * 301 + 2 + 10 + 4 + 57, "the file's bound");
static_assert(FILE_EXTRA == 8 + 25 + 12 + 12 && IDAT_AT == 8 + 25 + 8, "the chunk layout");
static_assert(base64_bytes(1) == 4 && base64_bytes(3) == 4 && base64_bytes(4) == 8, "base64 with padding");
static_assert(payload_bytes(MAX_SIDE, MAX_SIDE, 4) < (1ull << 35), "sizes are 64-bit; a payload from 2^31 on is refused");

// The largest stream a deflated image may have and still be taken: one byte below the stored form
OCHIP_DF_HD bool takes_deflated(uint64_t stream_bits, uint64_t F, uint64_t &bytes)
{
    bytes = 2 + (stream_bits + 7) / 8 + 4;
    return bytes < stored_bytes(F);
}

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

// ---- tokens at runtime distances ------------------------------------------------------------------------------------------
OCHIP_DF_HD uint64_t token_bits_at(uint16_t mark, uint8_t byte, const uint32_t *codes, int &n, int dist_left, int dist_up)
{
    const int len = mark & MARK_LEN;
    if (len == 0)
    {
        const uint32_t c = codes[byte];
        n = (int)(c >> 16);
        return c & 0xFFFF;
    }
    int eb, ev, db, dv;
    const uint32_t lc = codes[length_symbol(len, eb, ev)];
    const uint32_t dc = codes[NUM_LIT + distance_symbol((mark & MARK_UP) ? dist_up : dist_left, db, dv)];
    uint64_t v = lc & 0xFFFF;
    n = (int)(lc >> 16);
    v |= (uint64_t)ev << n, n += eb;
    v |= (uint64_t)(dc & 0xFFFF) << n, n += (int)(dc >> 16);
    v |= (uint64_t)dv << n, n += db;
    return v;
}

OCHIP_DF_HD int token_symbols_at(uint16_t mark, uint8_t byte, int &dist_sym, int dist_left, int dist_up)
{
    const int len = mark & MARK_LEN;
    dist_sym = -1;
    if (len == 0)
        return byte;
    int eb, ev;
    dist_sym = distance_symbol((mark & MARK_UP) ? dist_up : dist_left, eb, ev);
    return length_symbol(len, eb, ev);
}

// Byte o of the stored form of a payload of F bytes whose Adler-32 is `adler`; o < stored_bytes(F)
OCHIP_DF_HD uint8_t stored_byte_of(uint64_t o, const uint8_t *payload, uint64_t F, uint32_t adler)
{
    const uint64_t S = stored_bytes(F), blocks = (F + STORED_BLOCK - 1) / STORED_BLOCK;
    if (o < 2)
        return o == 0 ? 0x78 : 0x9C;
    if (o >= S - 4)
        return (uint8_t)(adler >> (8 * (S - 1 - o)));
    const uint64_t k = (o - 2) / (STORED_BLOCK + 5), r = (o - 2) % (STORED_BLOCK + 5);
    if (r >= 5)
        return payload[k * STORED_BLOCK + (r - 5)];
    const uint32_t len = k + 1 < blocks ? (uint32_t)STORED_BLOCK : (uint32_t)(F - k * STORED_BLOCK);
    return r == 0 ? (k + 1 == blocks ? 1 : 0) : r == 1 ? (uint8_t)len : r == 2 ? (uint8_t)(len >> 8) : r == 3 ? (uint8_t)~len : (uint8_t)(~len >> 8);
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

struct block_out
{
    uint32_t codes[NUM_SYMS];
    uint32_t header[HEADER_WORDS];
    uint32_t header_bits = 0, bits = 0;
};

// One segment of a payload: the candidate runs backwards from its end, the greedy parse from its start, the block's codes
inline void segment_block(const uint8_t *a, const shape &s, uint32_t seg, uint16_t *marks, block_out &B)
{
    const int64_t lo = (int64_t)seg * SEGMENT, hi = lo + SEGMENT < (int64_t)s.F ? lo + SEGMENT : (int64_t)s.F;
    const int64_t dl = s.c, du = s.stride;
    const bool use_up = s.stride <= UP_LIMIT;
    int left = 0, up = 0;
    for (int64_t p = hi - 1; p >= lo; p--)
    {
        left = p >= dl && a[p] == a[p - dl] ? left + 1 : 0;
        up = use_up && p >= du && a[p] == a[p - du] ? up + 1 : 0;
        marks[p] = choose_match(left, up);
    }
    block_work W;
    std::memset(W.counts, 0, sizeof W.counts);
    for (int64_t p = lo; p < hi;)
    {
        marks[p] |= MARK_START;
        int ds;
        W.counts[token_symbols_at(marks[p], a[p], ds, (int)dl, (int)du)]++;
        if (ds >= 0)
            W.counts[NUM_LIT + ds]++;
        const int len = marks[p] & MARK_LEN;
        p += len ? len : 1;
    }
    std::memset(B.header, 0, sizeof B.header);
    B.bits = build_block(W, seg + 1 == s.segs, B.codes, B.header, B.header_bits);
}

// Bits LSB first into zeroed bytes, the position 64-bit
struct bit_sink
{
    uint8_t *bytes;
    uint64_t cap_bits, bits;
    void put(uint64_t v, int n) // n <= 48
    {
        if (n <= 0 || bits + (uint64_t)n > cap_bits)
            return;
        uint64_t at = bits >> 3;
        const int s = (int)(bits & 7);
        bits += (uint64_t)n;
        unsigned __int128 w = (unsigned __int128)v << s;
        for (int left = n + s; left > 0; left -= 8, w >>= 8)
            bytes[at++] |= (uint8_t)w;
    }
};

inline void emit_segment(bit_sink &w, const uint8_t *a, const shape &s, uint32_t seg, const uint16_t *marks, const block_out &B)
{
    const int64_t lo = (int64_t)seg * SEGMENT, hi = lo + SEGMENT < (int64_t)s.F ? lo + SEGMENT : (int64_t)s.F;
    for (uint32_t b = 0; b < B.header_bits; b += 16)
    {
        const int n = B.header_bits - b < 16 ? (int)(B.header_bits - b) : 16;
        w.put((B.header[b >> 5] >> (b & 31)) & ((1u << n) - 1), n);
    }
    for (int64_t p = lo; p < hi; p++)
        if (marks[p] & MARK_START)
        {
            int n;
            const uint64_t v = token_bits_at(marks[p], a[p], B.codes, n, (int)s.c, (int)s.stride);
            w.put(v, n);
        }
    w.put(B.codes[EOB] & 0xFFFF, (int)(B.codes[EOB] >> 16));
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

// The file of a payload whose segments are marked and coded; out is cleared first
inline void assemble_file(const uint8_t *a, const shape &s, const uint16_t *marks, const block_out *blocks, std::vector<uint8_t> &out)
{
    uint64_t bits = 0;
    for (uint32_t k = 0; k < s.segs; k++)
        bits += blocks[k].bits;
    uint64_t zlen = 0;
    const bool deflated = takes_deflated(bits, s.F, zlen);
    if (!deflated)
        zlen = s.S;
    // the Adler-32 from the segments' partials, as the device combines them
    uint32_t a1 = 1, a2 = 0;
    for (uint32_t k = 0; k < s.segs; k++)
    {
        const uint64_t lo = (uint64_t)k * SEGMENT, n = s.F - lo < (uint64_t)SEGMENT ? s.F - lo : (uint64_t)SEGMENT;
        const uint32_t ad = adler32(a + lo, (size_t)n);
        adler_combine(a1, a2, ad & 0xFFFF, ad >> 16, (uint32_t)n);
    }
    const uint32_t adler = a2 << 16 | a1;
    out.assign((size_t)(zlen + FILE_EXTRA), 0);
    uint8_t *z = out.data() + IDAT_AT;
    if (deflated)
    {
        z[0] = 0x78, z[1] = 0x9C;
        bit_sink w{z, (zlen - 4) * 8, 16};
        for (uint32_t k = 0; k < s.segs; k++)
            emit_segment(w, a, s, k, marks, blocks[k]);
        put_be32(z + zlen - 4, adler);
    }
    else
        for (uint64_t o = 0; o < zlen; o++)
            z[o] = stored_byte_of(o, a, s.F, adler);
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
        segment_block(payload.data(), s, k, marks.data(), blocks[k]);
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
