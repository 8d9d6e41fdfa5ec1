// Baseline JPEG of the textured OBJ's texture (the reference's cv::imwrite(jpg_path, texture),
// src/ortho/ortho.cpp:2096-2123): 8-bit YCbCr 4:2:0, the Annex K tables scaled by the quality, libjpeg's integer "islow"
// forward DCT, no restart intervals - the bytes libjpeg-turbo writes with cv::imwrite's default settings.  This header is the
// arithmetic for both routes: the tables, the sample and edge rules, the transform, the quantiser, the entropy coder over a
// bit sink, the file's header and tail, and the row bookkeeping of an encoder fed band by band.  csrc/jpeg_encode.hip runs it
// in kernels, host/jpeg_encode.cpp in loops; it includes nothing of either, so a stand-alone program builds from it.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define OCHIP_JPEG_HD __host__ __device__ inline
#else
#define OCHIP_JPEG_HD inline
#endif

namespace ochip_jp
{

constexpr int64_t MAX_DIMENSION = 65500; // libjpeg's JPEG_MAX_DIMENSION
constexpr int MCU_SIDE = 16, MCU_BLOCKS = 6, MCU_COEFS = MCU_BLOCKS * 64;
// before stuffing a block is at most 20 bits of DC and 63 x 26 bits of ACs: 1 658 bits, an MCU 9 948 bits = 1 244 bytes
constexpr int BLOCK_MAX_BITS = 20 + 63 * 26;
constexpr int MCU_MAX_BYTES = (MCU_BLOCKS * BLOCK_MAX_BITS + 7) / 8;
static_assert(MCU_MAX_BYTES == 1244, "the bound every buffer is sized from");

// What the kernels and loops read: built once per encoder on the host (build_tables), uploaded as it lies here.
struct tables
{
    uint16_t qdiv[2][64]; // 8 x the quantisation entry, natural (row-major) order; [0] luma, [1] chroma
    uint8_t zz[64];       // zigzag position -> natural index
    uint8_t qzz[2][64];   // the entries in zigzag order, as the DQT markers carry them
    uint32_t dc[2][12];   // length << 16 | code by category
    uint32_t ac[2][256];  // length << 16 | code by run << 4 | size
};

struct geometry
{
    int32_t w = 0, h = 0;
    int32_t mw = 0, mh = 0;   // MCU columns and rows
    int32_t ybw = 0, ybh = 0; // real luma blocks; the chroma planes' real blocks are the MCU grid itself
};

inline geometry make_geometry(int64_t w, int64_t h)
{
    geometry g;
    g.w = (int32_t)w, g.h = (int32_t)h;
    g.mw = (int32_t)((w + 15) / 16), g.mh = (int32_t)((h + 15) / 16);
    g.ybw = (int32_t)((w + 7) / 8), g.ybh = (int32_t)((h + 7) / 8);
    return g;
}

// Rows of pixels from two places: the rows kept from the feeds before (carry, from row carry_row0 on) and the band being
// fed (from row band_row0 on).  A pixel is `stride` bytes, channels 0, 1, 2 are R, G, B.
struct rows_view
{
    const uint8_t *carry = nullptr;
    const uint8_t *band = nullptr;
    int64_t carry_row0 = 0, band_row0 = 0;
    int32_t carry_stride = 4, band_stride = 4;
    int32_t w = 0;
    OCHIP_JPEG_HD const uint8_t *at(int64_t y, int64_t x) const
    {
        return y < band_row0 ? carry + ((size_t)(y - carry_row0) * (size_t)w + (size_t)x) * (size_t)carry_stride
                             : band + ((size_t)(y - band_row0) * (size_t)w + (size_t)x) * (size_t)band_stride;
    }
};

OCHIP_JPEG_HD void rgb_to_ycc(int r, int g, int b, int &y, int &cb, int &cr)
{
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The luma sample at (x, y) of the padded plane: the last column and the last row repeat.
OCHIP_JPEG_HD int luma_sample(const rows_view &v, const geometry &g, int64_t x, int64_t y)
{
    const uint8_t *p = v.at(y < g.h ? y : g.h - 1, x < g.w ? x : g.w - 1);
    int Y, cb, cr;
    rgb_to_ycc(p[0], p[1], p[2], Y, cb, cr);
    return Y;
}

// The chroma samples at (cx, cy) of the padded half-size planes.  The last column repeats before the 2 x 2 average, the last
// row only up to an even height; below that the averaged last row repeats.  The bias alternates 1, 2 along a row.
OCHIP_JPEG_HD void chroma_sample(const rows_view &v, const geometry &g, int64_t cx, int64_t cy, int &cb_out, int &cr_out)
{
    const int64_t last_cy = (g.h + 1) / 2 - 1, c = cy < last_cy ? cy : last_cy;
    const int64_t y0 = 2 * c, y1 = 2 * c + 1 < g.h ? 2 * c + 1 : g.h - 1;
    const int64_t x0 = 2 * cx < g.w ? 2 * cx : g.w - 1, x1 = 2 * cx + 1 < g.w ? 2 * cx + 1 : g.w - 1;
    int sb = 0, sr = 0;
    const int64_t ys[2] = {y0, y1}, xs[2] = {x0, x1};
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
        {
            const uint8_t *p = v.at(ys[i], xs[j]);
            int Y, cb, cr;
            rgb_to_ycc(p[0], p[1], p[2], Y, cb, cr);
            sb += cb, sr += cr;
        }
    const int bias = (cx & 1) ? 2 : 1;
    cb_out = (sb + bias) >> 2, cr_out = (sr + bias) >> 2;
}

OCHIP_JPEG_HD int descale(int x, int n)
{
    return (x + (1 << (n - 1))) >> n;
}

// One 8-point pass of libjpeg's jfdctint (13 constant bits, 2 pass-1 bits) in place; d is indexed by constants only.
template <bool FIRST> OCHIP_JPEG_HD void fdct8(int (&d)[8])
{
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST)
        d[0] = (t10 + t11) * 4, d[4] = (t10 - t11) * 4;
    else
        d[0] = descale(t10 + t11, 2), d[4] = descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, N);
    d[6] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
    z3 += z5, z4 += z5;
    d[7] = descale(a4 + z1 + z3, N);
    d[5] = descale(a5 + z2 + z4, N);
    d[3] = descale(a6 + z2 + z3, N);
    d[1] = descale(a7 + z1 + z4, N);
}

// c: a transformed coefficient (8 x the true one), d: 8 x the table entry
OCHIP_JPEG_HD int quantise(int c, int d)
{
    const int t = ((c < 0 ? -c : c) + (d >> 1)) / d;
    return c < 0 ? -t : t;
}

OCHIP_JPEG_HD int bit_length(uint32_t v)
{
    return v ? 32 - __builtin_clz(v) : 0;
}

// The entropy coder of one block over a sink with put(bits, length), length <= 27.  dc(diff), then ac(v) for the 63
// coefficients in zigzag order, then end().
template <class Sink> struct block_coder
{
    Sink &sink;
    const uint32_t *dc_table, *ac_table;
    int run = 0;
    OCHIP_JPEG_HD block_coder(Sink &s, const uint32_t *dct, const uint32_t *act) : sink(s), dc_table(dct), ac_table(act) {}
    OCHIP_JPEG_HD void value(uint32_t entry, int v, int nb)
    {
        const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u);
        sink.put(((entry & 0xFFFFu) << nb) | low, (int)(entry >> 16) + nb);
    }
    OCHIP_JPEG_HD void dc(int diff)
    {
        const int nb = bit_length((uint32_t)(diff < 0 ? -diff : diff));
        value(dc_table[nb], diff, nb);
    }
    OCHIP_JPEG_HD void ac(int v)
    {
        if (v == 0)
        {
            run++;
            return;
        }
        while (run > 15)
        {
            const uint32_t zrl = ac_table[0xF0];
            sink.put(zrl & 0xFFFFu, (int)(zrl >> 16));
            run -= 16;
        }
        const int nb = bit_length((uint32_t)(v < 0 ? -v : v));
        value(ac_table[(run << 4) | nb], v, nb);
        run = 0;
    }
    OCHIP_JPEG_HD void end()
    {
        if (run)
        {
            const uint32_t eob = ac_table[0];
            sink.put(eob & 0xFFFFu, (int)(eob >> 16));
        }
    }
};

struct bit_counter
{
    uint32_t bits = 0;
    OCHIP_JPEG_HD void put(uint32_t, int len)
    {
        bits += (uint32_t)len;
    }
};

// Which luma blocks of the MCU at (mx, my) exist; a dummy block carries the DC of the block coded before it and no AC.
OCHIP_JPEG_HD bool luma_block_real(const geometry &g, int mx, int my, int b)
{
    return 2 * mx + (b & 1) < g.ybw && 2 * my + (b >> 1) < g.ybh;
}

// ---- host only from here on ------------------------------------------------------------------------------------------------

namespace annex_k
{
const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
} // namespace annex_k

inline void huffman_codes(const uint8_t *bits16, const uint8_t *vals, uint32_t *by_symbol)
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++)
    {
        for (int i = 0; i < bits16[len - 1]; i++)
            by_symbol[vals[k++]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
}

// quality 1 .. 100
inline void build_tables(int quality, tables &t)
{
    std::memset(&t, 0, sizeof t);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; c++)
    {
        for (int i = 0; i < 64; i++)
        {
            int e = (annex_k::QUANT[c][i] * scale + 50) / 100;
            e = e < 1 ? 1 : e > 255 ? 255 : e;
            t.qdiv[c][i] = (uint16_t)(8 * e);
        }
        for (int k = 0; k < 64; k++)
            t.qzz[c][k] = (uint8_t)(t.qdiv[c][annex_k::ZIGZAG[k]] / 8);
        huffman_codes(annex_k::DC_BITS[c], annex_k::DC_VALS, t.dc[c]);
        huffman_codes(annex_k::AC_BITS[c], annex_k::AC_VALS[c], t.ac[c]);
    }
    std::memcpy(t.zz, annex_k::ZIGZAG, 64);
}

// Everything of the file ahead of the entropy-coded data
inline void append_header(std::vector<uint8_t> &out, const geometry &g, const tables &t)
{
    auto bytes = [&out](std::initializer_list<int> l) {
        for (int b : l)
            out.push_back((uint8_t)b);
    };
    bytes({0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; c++)
    {
        bytes({0xFF, 0xDB, 0x00, 0x43, c});
        out.insert(out.end(), t.qzz[c], t.qzz[c] + 64);
    }
    bytes({0xFF, 0xC0, 0x00, 0x11, 0x08, g.h >> 8, g.h & 255, g.w >> 8, g.w & 255, 0x03, 0x01, 0x22, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01});
    for (int k = 0; k < 4; k++) // DC0, AC0, DC1, AC1
    {
        const int c = k >> 1, ac = k & 1, n = ac ? 162 : 12;
        bytes({0xFF, 0xC4, (3 + 16 + n) >> 8, (3 + 16 + n) & 255, ac << 4 | c});
        const uint8_t *b = ac ? annex_k::AC_BITS[c] : annex_k::DC_BITS[c], *v = ac ? annex_k::AC_VALS[c] : annex_k::DC_VALS;
        out.insert(out.end(), b, b + 16);
        out.insert(out.end(), v, v + n);
    }
    bytes({0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00});
}

// The end of the file: the last partial byte (nbits of `partial`, 0 .. 7) filled with 1-bits and stuffed, then EOI
inline void append_tail(std::vector<uint8_t> &out, uint32_t partial, int nbits)
{
    if (nbits > 0)
    {
        const uint8_t b = (uint8_t)((partial << (8 - nbits)) | ((1u << (8 - nbits)) - 1u));
        out.push_back(b);
        if (b == 0xFF)
            out.push_back(0);
    }
    out.push_back(0xFF), out.push_back(0xD9);
}

// The rows an encoder has taken and what a feed does with them.  Rows arrive in ascending contiguous bands of any count;
// an MCU row is encoded once its 16 rows are there (the last one once the raster's last row is), the rows behind the last
// complete MCU row - 15 at most - are kept for the next feed.
struct progress
{
    int64_t height = 0;
    int64_t next_row = 0; // rows fed
    int64_t done_rows = 0; // rows encoded: a multiple of 16, or height
    bool finished = false;

    struct plan
    {
        int64_t mcu_row0 = 0, mcu_rows = 0; // to encode now
        int64_t keep_from = 0, keep_rows = 0; // rows [keep_from, keep_from + keep_rows) of the band go behind ...
        int64_t keep_at = 0;                  // ... carried row keep_at (0: the carry starts anew at keep_from)
    };
    // "" and the plan, or the refusal; nothing changes on a refusal
    std::string feed(int64_t row0, int64_t rows, plan &p)
    {
        const std::string band = "rows " + std::to_string(row0) + " to " + std::to_string(row0 + rows);
        if (finished)
            return band + " after finish";
        if (rows <= 0 || row0 < 0)
            return band + ": a band has at least one row";
        if (row0 > next_row)
            return "gap: " + band + " when row " + std::to_string(next_row) + " is next";
        if (row0 < next_row)
            return "overlap: " + band + " when row " + std::to_string(next_row) + " is next";
        if (row0 + rows > height)
            return band + " of a raster of " + std::to_string(height) + " rows";
        const int64_t end = row0 + rows;
        const int64_t upto = end == height ? height : end / 16 * 16; // rows encoded after this feed
        p.mcu_row0 = done_rows / 16, p.mcu_rows = upto > done_rows ? (upto - done_rows + 15) / 16 : 0;
        if (p.mcu_rows > 0)
            p.keep_from = upto, p.keep_rows = end - upto, p.keep_at = 0;
        else
            p.keep_from = row0, p.keep_rows = rows, p.keep_at = row0 - done_rows;
        next_row = end;
        if (p.mcu_rows > 0)
            done_rows = upto;
        return "";
    }
    std::string finish()
    {
        if (finished)
            return "finish after finish";
        if (next_row != height)
            return "finish at row " + std::to_string(next_row) + " of " + std::to_string(height);
        finished = true;
        return "";
    }
};

// The encoded bytes the caller has not collected yet
struct byte_stream
{
    std::vector<uint8_t> bytes;
    // "" or the refusal; buf == NULL: the count alone
    std::string collect(uint8_t *buf, uint64_t cap, uint64_t *n)
    {
        *n = bytes.size();
        if (!buf)
            return "";
        if (cap < bytes.size())
            return std::to_string(bytes.size()) + " bytes are ready, the capacity is " + std::to_string(cap);
        if (!bytes.empty())
            std::memcpy(buf, bytes.data(), bytes.size());
        bytes.clear();
        return "";
    }
};

inline std::string refuse_create(int64_t width, int64_t height, int quality)
{
    if (width < 1 || height < 1 || width > MAX_DIMENSION || height > MAX_DIMENSION)
        return "a raster of " + std::to_string(width) + " x " + std::to_string(height) + ", each side is 1 .. " + std::to_string(MAX_DIMENSION);
    if (quality < 1 || quality > 100)
        return "quality " + std::to_string(quality) + " is not 1 .. 100";
    return "";
}

} // namespace ochip_jp
