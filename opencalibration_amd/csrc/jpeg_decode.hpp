// Baseline JPEG decoding of the load stage (the reference's cv::imread(path),
// src/extract/extract_image.cpp:18-21): the pixels libjpeg-turbo's default decode gives - the "islow" inverse DCT, the
// triangle ("fancy") chroma upsampling, the 16-bit fixed-point colour conversion, B, G, R order - and the EXIF orientation
// cv::imread applies.  This header is the rules of both routes: the header parser, the Huffman tables as they are read, the
// bit reader over a stuffed scan, the symbol walk with its state, the transform, the upsampling filters, the colour
// conversion and the orientation map.  csrc/jpeg_decode.hip runs it in kernels, host/jpeg_decode.cpp in loops; it includes
// nothing of either, so a stand-alone program builds from it.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define OCHIP_JD_HD __host__ __device__ inline
#else
#define OCHIP_JD_HD inline
#endif

namespace ochip_jd
{

enum status : int32_t
{
    OK = 0,
    UNSUPPORTED = 1, // a JPEG this decoder does not take: the caller falls back
    CORRUPT = 2      // truncated or not decodable
};

constexpr int MIN_SUBSEQUENCE_BITS = 32;    // the smallest subsequence the scheme admits (a multiple of 32)
constexpr int DEFAULT_SUBSEQUENCE_BITS = 1024;
constexpr int LOOK_BITS = 9;
constexpr int64_t MAX_BATCH_FILES = 65535; // the device route spreads a batch over a grid dimension

// One Huffman table as both routes read it: codes of up to LOOK_BITS bits by direct lookup, the longer ones by the
// canonical comparison against the largest code of each length.
struct huffman
{
    uint16_t look[1 << LOOK_BITS]; // length << 8 | symbol; length 0: a longer code
    int32_t maxcode[18];           // the largest code of a length, -1: none; [17] ends every search
    int32_t valoff[17];            // index of the first symbol of a length minus its first code
    uint8_t vals[256];
};

// What the kernels and loops read of one file, built by parse(), uploaded as it lies here
struct tables
{
    uint16_t quant[3][64]; // per component, natural (row-major) order
    huffman dc[3], ac[3];  // per component
    uint8_t zz[64];        // zigzag position -> natural index
};

struct geometry
{
    int32_t w = 0, h = 0;    // the file's own, before the orientation
    int32_t ncomp = 0;       // 1 or 3
    int32_t hs = 1, vs = 1;  // luma sampling factors: 1x1, 2x1, 2x2; chroma is 1x1
    int32_t mw = 0, mh = 0;  // MCU columns and rows
    int32_t bpm = 1;         // blocks per MCU
    int32_t ri = 0;          // restart interval in MCUs, 0: none
    int32_t orientation = 1; // EXIF tag 0x0112, 1 .. 8
    int32_t cw = 0, ch = 0;  // the chroma planes' own (downsampled) width and height
    OCHIP_JD_HD int32_t yw() const // the padded planes
    {
        return mw * 8 * hs;
    }
    OCHIP_JD_HD int32_t yh() const
    {
        return mh * 8 * vs;
    }
    OCHIP_JD_HD int32_t pcw() const
    {
        return mw * 8;
    }
    OCHIP_JD_HD int32_t pch() const
    {
        return mh * 8;
    }
};

// ---- the bit reader ---------------------------------------------------------------------------------------------------------
// Positions are bit positions in the file's bytes (8 x byte + bit, the most significant bit first) and always name a bit of
// a data byte: the 00 behind an FF is stepped over when a byte is left, never pointed at.  Bytes at or past `end` read as 0,
// so a walk in a wrong state never leaves the scan.
struct bit_reader
{
    const uint8_t *d;
    uint32_t end; // byte index
    OCHIP_JD_HD uint32_t byte(uint32_t i) const
    {
        return i < end ? d[i] : 0u;
    }
    OCHIP_JD_HD uint32_t next_byte(uint32_t i) const
    {
        return byte(i) == 0xFFu ? i + 2 : i + 1;
    }
    // 32 bits from pos on
    OCHIP_JD_HD uint32_t peek32(uint32_t pos) const
    {
        uint32_t i = pos >> 3;
        uint64_t acc = 0;
        for (int k = 0; k < 5; k++)
        {
            acc = acc << 8 | byte(i);
            i = next_byte(i);
        }
        return (uint32_t)(acc >> (8 - (pos & 7)));
    }
    OCHIP_JD_HD uint32_t skip(uint32_t pos, int n) const
    {
        uint32_t i = pos >> 3;
        int bit = (int)(pos & 7) + n;
        while (bit >= 8)
        {
            i = next_byte(i);
            bit -= 8;
        }
        return i << 3 | (uint32_t)bit;
    }
    // the first data bit at or behind byte i of a scan that starts at byte i0
    OCHIP_JD_HD uint32_t normalise(uint32_t i, uint32_t i0) const
    {
        return (i > i0 && byte(i - 1) == 0xFFu && byte(i) == 0u ? i + 1 : i) << 3;
    }
};

// ---- the symbol walk --------------------------------------------------------------------------------------------------------
// The state between two symbols: the next symbol starts at bit `pos`, belongs to block `blk` of its MCU and codes the
// coefficient at zigzag index `zz` (0: the DC difference).
struct walk_state
{
    uint32_t pos;
    uint8_t blk, zz;
    OCHIP_JD_HD uint64_t packed() const
    {
        return (uint64_t)pos << 16 | (uint64_t)blk << 8 | zz;
    }
    static OCHIP_JD_HD walk_state unpacked(uint64_t v)
    {
        walk_state s;
        s.pos = (uint32_t)(v >> 16), s.blk = (uint8_t)(v >> 8), s.zz = (uint8_t)v;
        return s;
    }
};

OCHIP_JD_HD int component_of_block(const geometry &g, int blk)
{
    const int luma = g.hs * g.vs;
    return g.ncomp == 1 || blk < luma ? 0 : blk - luma + 1;
}

struct symbol
{
    int zz;    // where the value goes (0: DC difference), -1: no value (end of block, run of 16)
    int value;
    bool block_done;
    bool bad; // a code no table has, a category past 11, an index past 63, bits past the scan's end
};

// One symbol from state s, which it advances.  Every input has a defined successor: a code no table has counts as 16 bits
// of an end of block, an index past 63 ends the block.  `bad` tells the final pass that the stream is not a JPEG's.
OCHIP_JD_HD symbol next_symbol(const bit_reader &r, const tables &t, const geometry &g, walk_state &s, uint32_t end_bit)
{
    symbol out;
    out.zz = -1, out.value = 0, out.block_done = false, out.bad = false;
    const int c = component_of_block(g, s.blk);
    const huffman &h = s.zz == 0 ? t.dc[c] : t.ac[c];
    const uint32_t bits = r.peek32(s.pos), top = bits >> 16;
    int len = h.look[top >> (16 - LOOK_BITS)] >> 8, sym = h.look[top >> (16 - LOOK_BITS)] & 255;
    if (len == 0)
    {
        len = LOOK_BITS + 1;
        while (len <= 16 && (int32_t)(top >> (16 - len)) > h.maxcode[len])
            len++;
        if (len > 16)
            len = 16, sym = 0, out.bad = true;
        else
            sym = h.vals[(h.valoff[len] + (int32_t)(top >> (16 - len))) & 255];
    }
    const int size = sym & 15, run = sym >> 4;
    int value = 0;
    if (size)
    {
        const int raw = (int)((bits << len) >> (32 - size));
        value = raw < (1 << (size - 1)) ? raw - (1 << size) + 1 : raw;
    }
    s.pos = r.skip(s.pos, len + size);
    if (s.pos > end_bit)
        out.bad = true;
    if (s.zz == 0)
    {
        if (sym > 11)
            out.bad = true;
        out.zz = 0, out.value = value;
        s.zz = 1;
    }
    else if (size == 0)
    {
        if (run == 15)
            s.zz = (uint8_t)(s.zz + 16);
        else
        {
            if (run != 0)
                out.bad = true;
            s.zz = 64;
        }
        if (s.zz > 64)
            out.bad = true;
    }
    else
    {
        const int at = s.zz + run;
        if (at > 63)
            out.bad = true, s.zz = 64;
        else
            out.zz = at, out.value = value, s.zz = (uint8_t)(at + 1);
    }
    if (s.zz >= 64)
    {
        out.block_done = true;
        s.zz = 0;
        s.blk = (uint8_t)(s.blk + 1 == g.bpm ? 0 : s.blk + 1);
    }
    return out;
}

// ---- dequantise and the inverse transform -----------------------------------------------------------------------------------
OCHIP_JD_HD int descale(int x, int n)
{
    return (x + (1 << (n - 1))) >> n;
}

// One 8-point pass of libjpeg's jidctint (13 constant bits, 2 pass-1 bits) in place
template <bool FIRST> OCHIP_JD_HD void idct8(int (&d)[8])
{
    constexpr int N = FIRST ? 11 : 18;
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
    z2 = d[0], z3 = d[4];
    int tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7], tmp1 = d[5], tmp2 = d[3], tmp3 = d[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    d[0] = descale(tmp10 + tmp3, N), d[7] = descale(tmp10 - tmp3, N);
    d[1] = descale(tmp11 + tmp2, N), d[6] = descale(tmp11 - tmp2, N);
    d[2] = descale(tmp12 + tmp1, N), d[5] = descale(tmp12 - tmp1, N);
    d[3] = descale(tmp13 + tmp0, N), d[4] = descale(tmp13 - tmp0, N);
}

OCHIP_JD_HD int clamp255(int v)
{
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// The dequantised coefficient as the 16-bit lanes of libjpeg-turbo's transform hold it
OCHIP_JD_HD int dequantise(int coef, int q)
{
    return (int16_t)(coef * q);
}

// ---- upsampling, colour, orientation ----------------------------------------------------------------------------------------
// A full-resolution chroma sample at (x, y) from a padded plane of row length `stride`.  The triangle filters apply where
// the plane's own width exceeds 2 (libjpeg chooses replication below that); their first / last column rules hold at the
// plane's own width cw, the row context repeats the rows 0 and ch - 1.
OCHIP_JD_HD int chroma_at(const uint8_t *plane, int stride, const geometry &g, int x, int y)
{
    if (g.hs == 1)
        return plane[(size_t)y * stride + x];
    const int cx = x >> 1;
    const bool fancy = g.cw > 2;
    if (g.vs == 1)
    {
        const uint8_t *row = plane + (size_t)y * stride;
        if (!fancy)
            return row[cx];
        const int v = row[cx];
        if (x & 1)
            return cx == g.cw - 1 ? v : (3 * v + row[cx + 1] + 2) >> 2;
        return cx == 0 ? v : (3 * v + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    if (!fancy)
        return plane[(size_t)cy * stride + cx];
    int oy = (y & 1) ? cy + 1 : cy - 1;
    oy = oy < 0 ? 0 : oy > g.ch - 1 ? g.ch - 1 : oy;
    const uint8_t *near = plane + (size_t)cy * stride, *far = plane + (size_t)oy * stride;
    const int here = 3 * near[cx] + far[cx];
    if (x & 1)
        return cx == g.cw - 1 ? (4 * here + 7) >> 4 : (3 * here + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * here + 8) >> 4 : (3 * here + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

OCHIP_JD_HD void ycc_to_bgr(int y, int cb, int cr, uint8_t *bgr)
{
    cb -= 128, cr -= 128;
    bgr[2] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
    bgr[1] = (uint8_t)clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    bgr[0] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
}

// Where pixel (x, y) of a w x h picture goes under an EXIF orientation, and the oriented picture's size
OCHIP_JD_HD void oriented(int orientation, int w, int h, int x, int y, int &ox, int &oy)
{
    switch (orientation)
    {
    case 2: ox = w - 1 - x, oy = y; break;
    case 3: ox = w - 1 - x, oy = h - 1 - y; break;
    case 4: ox = x, oy = h - 1 - y; break;
    case 5: ox = y, oy = x; break;
    case 6: ox = h - 1 - y, oy = x; break;
    case 7: ox = h - 1 - y, oy = w - 1 - x; break;
    case 8: ox = y, oy = w - 1 - x; break;
    default: ox = x, oy = y;
    }
}

OCHIP_JD_HD int oriented_width(int orientation, int w, int h)
{
    return orientation >= 5 && orientation <= 8 ? h : w;
}

// Block n of an MCU-ordered scan: its component and the block's column and row in that component's padded plane
OCHIP_JD_HD void place_block(const geometry &g, uint32_t n, int &comp, int &bx, int &by)
{
    const int mcu = (int)(n / (uint32_t)g.bpm), j = (int)(n % (uint32_t)g.bpm);
    const int mx = mcu % g.mw, my = mcu / g.mw;
    comp = component_of_block(g, j);
    if (comp == 0)
        bx = mx * g.hs + j % g.hs, by = my * g.vs + j / g.hs;
    else
        bx = mx, by = my;
}

// The 64 samples of a block from its coefficients (natural order), rows of 8: both passes in one call, the host's way
inline void idct_block(const int16_t *coef, const uint16_t *q, uint8_t *out, int stride)
{
    int ws[64];
    for (int c = 0; c < 8; c++)
    {
        int d[8];
        for (int r = 0; r < 8; r++)
            d[r] = dequantise(coef[r * 8 + c], q[r * 8 + c]);
        idct8<true>(d);
        for (int r = 0; r < 8; r++)
            ws[r * 8 + c] = d[r];
    }
    for (int r = 0; r < 8; r++)
    {
        int d[8];
        for (int c = 0; c < 8; c++)
            d[c] = ws[r * 8 + c];
        idct8<false>(d);
        for (int c = 0; c < 8; c++)
            out[(size_t)r * stride + c] = (uint8_t)clamp255(d[c] + 128);
    }
}

// ---- host only from here on: the header parser ------------------------------------------------------------------------------

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// A restart interval's bytes [byte0, byte1) and its first MCU; a file without DRI has one
struct interval
{
    uint32_t byte0, byte1, first_mcu;
};

struct parsed
{
    int32_t status = CORRUPT;
    geometry g;
    tables t;
    uint32_t scan0 = 0, scan1 = 0; // the entropy-coded bytes
    std::vector<interval> intervals;
    uint32_t mcus() const
    {
        return (uint32_t)g.mw * (uint32_t)g.mh;
    }
};

// false: the counts do not describe a prefix code
inline bool build_huffman(const uint8_t *bits16, const uint8_t *vals, int nvals, huffman &h)
{
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.vals, vals, (size_t)nvals);
    int32_t code = 0, k = 0;
    for (int len = 1; len <= 16; len++)
    {
        if (code + bits16[len - 1] > (1 << len)) // more codes of this length than there are: refused before any store
            return false;
        h.valoff[len] = k - code;
        for (int i = 0; i < bits16[len - 1]; i++, k++, code++)
            if (len <= LOOK_BITS)
                for (int f = 0; f < 1 << (LOOK_BITS - len); f++)
                    h.look[(code << (LOOK_BITS - len)) | f] = (uint16_t)(len << 8 | vals[k]);
        h.maxcode[len] = bits16[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7FFFFFFF;
    return true;
}

inline uint32_t be16(const uint8_t *p)
{
    return (uint32_t)p[0] << 8 | p[1];
}

// EXIF tag 0x0112 of an APP1 payload ("Exif\0\0" and a TIFF header in either byte order); 1 when there is none
inline int exif_orientation(const uint8_t *p, size_t n)
{
    if (n < 14 || std::memcmp(p, "Exif\0\0", 6) != 0)
        return 0;
    const uint8_t *t = p + 6;
    const size_t tn = n - 6;
    const bool le = t[0] == 'I' && t[1] == 'I';
    if (!le && !(t[0] == 'M' && t[1] == 'M'))
        return 0;
    auto u16 = [&](size_t at) -> uint32_t { return le ? (uint32_t)t[at] | (uint32_t)t[at + 1] << 8 : (uint32_t)t[at] << 8 | t[at + 1]; };
    auto u32 = [&](size_t at) -> uint32_t { return le ? u16(at) | u16(at + 2) << 16 : u16(at) << 16 | u16(at + 2); };
    if (u16(2) != 42)
        return 0;
    const size_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2)
        return 0;
    const size_t count = u16(ifd);
    for (size_t e = 0; e < count; e++)
    {
        const size_t at = ifd + 2 + 12 * e;
        if (at + 12 > tn)
            return 0;
        if (u16(at) == 0x0112)
        {
            const uint32_t v = u16(at + 2) == 3 ? u16(at + 8) : u16(at + 2) == 4 ? u32(at + 8) : 0;
            return v >= 1 && v <= 8 ? (int)v : 0;
        }
    }
    return 0;
}

// The headers of a file: markers, tables, geometry, the scan's extent and restart intervals, the orientation.  Reads no
// entropy-coded bit.  p.status: OK, or why the file is refused.
inline void parse(const uint8_t *d, size_t n, parsed &p)
{
    p = parsed();
    std::memcpy(p.t.zz, ZIGZAG, 64);
    if (n < 4 || n >= (1u << 28) || d[0] != 0xFF || d[1] != 0xD8)
        return;
    uint16_t quant[4][64];
    bool have_quant[4] = {false, false, false, false}, have_dc[4] = {false, false, false, false}, have_ac[4] = {false, false, false, false};
    std::vector<huffman> dc(4), ac(4);
    bool have_frame = false, unsupported = false;
    int comp_id[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
    int adobe_transform = -1;
    geometry &g = p.g;
    size_t at = 2;
    for (;;)
    {
        // a marker: FF, any number of fill FFs, the code
        if (at + 2 > n || d[at] != 0xFF)
            return;
        while (at < n && d[at] == 0xFF)
            at++;
        if (at >= n)
            return;
        const int m = d[at++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7))
            continue;
        if (m == 0xD9)
            return;
        if (at + 2 > n)
            return;
        const size_t len = be16(d + at);
        if (len < 2 || at + len > n)
            return;
        const uint8_t *s = d + at + 2;
        const size_t sn = len - 2;
        at += len;
        if (m == 0xC0 || m == 0xC1)
        {
            if (have_frame || sn < 6)
                return;
            have_frame = true;
            const int precision = s[0], nc = s[5];
            g.h = (int32_t)be16(s + 1), g.w = (int32_t)be16(s + 3);
            if (sn != (size_t)(6 + 3 * nc) || nc < 1)
                return;
            if (precision != 8 || (nc != 1 && nc != 3) || g.h == 0 || g.w == 0)
            {
                unsupported = true;
                g.ncomp = nc;
                continue;
            }
            g.ncomp = nc;
            for (int c = 0; c < nc; c++)
            {
                comp_id[c] = s[6 + 3 * c], comp_h[c] = s[7 + 3 * c] >> 4, comp_v[c] = s[7 + 3 * c] & 15, comp_q[c] = s[8 + 3 * c];
                if (comp_q[c] > 3 || comp_h[c] < 1 || comp_v[c] < 1)
                    return;
            }
        }
        else if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC) || m == 0xCC)
        {
            // progressive, lossless, differential, arithmetic coding (SOF9 .. SOF15, DAC)
            if (sn >= 6 && m != 0xCC)
                g.h = (int32_t)be16(s + 1), g.w = (int32_t)be16(s + 3), g.ncomp = s[5];
            p.status = UNSUPPORTED;
            return;
        }
        else if (m == 0xDB)
        {
            size_t o = 0;
            while (o < sn)
            {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (tq > 3 || pq > 1)
                    return;
                if (pq == 1)
                {
                    if (o + 1 + 128 > sn)
                        return;
                    unsupported = true;
                    o += 129;
                    continue;
                }
                if (o + 1 + 64 > sn)
                    return;
                for (int k = 0; k < 64; k++)
                    quant[tq][ZIGZAG[k]] = s[o + 1 + k];
                have_quant[tq] = true;
                o += 65;
            }
        }
        else if (m == 0xC4)
        {
            size_t o = 0;
            while (o < sn)
            {
                if (o + 17 > sn)
                    return;
                const int tc = s[o] >> 4, th = s[o] & 15;
                int count = 0;
                for (int i = 0; i < 16; i++)
                    count += s[o + 1 + i];
                if (tc > 1 || th > 3 || count > 256 || o + 17 + (size_t)count > sn)
                    return;
                if (!build_huffman(s + o + 1, s + o + 17, count, tc ? ac[th] : dc[th]))
                    return;
                (tc ? have_ac : have_dc)[th] = true;
                o += 17 + (size_t)count;
            }
        }
        else if (m == 0xDD)
        {
            if (sn != 2)
                return;
            g.ri = (int32_t)be16(s);
        }
        else if (m == 0xE1)
        {
            const int o = exif_orientation(s, sn);
            if (o)
                g.orientation = o;
        }
        else if (m == 0xEE)
        {
            if (sn >= 12 && std::memcmp(s, "Adobe", 5) == 0)
                adobe_transform = s[11];
        }
        else if (m == 0xDA)
        {
            if (!have_frame)
                return;
            if (unsupported)
            {
                p.status = UNSUPPORTED;
                return;
            }
            if (sn < 1)
                return;
            const int ns = s[0];
            if (sn != (size_t)(4 + 2 * ns))
                return;
            if (ns != g.ncomp)
            {
                p.status = UNSUPPORTED; // several scans
                return;
            }
            if (g.ncomp == 3)
            {
                const bool rgb_ids = comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B';
                const bool sampling = comp_h[1] == 1 && comp_v[1] == 1 && comp_h[2] == 1 && comp_v[2] == 1 &&
                                      ((comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2));
                if (adobe_transform == 0 || (adobe_transform < 0 && rgb_ids) || !sampling)
                {
                    p.status = UNSUPPORTED;
                    return;
                }
                g.hs = comp_h[0], g.vs = comp_v[0];
            }
            else
                g.hs = g.vs = 1; // a single component is not interleaved: its blocks come one by one
            for (int c = 0; c < ns; c++)
            {
                const int id = s[1 + 2 * c], td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (id != comp_id[c])
                {
                    p.status = UNSUPPORTED; // another component order
                    return;
                }
                if (td > 3 || ta > 3 || !have_dc[td] || !have_ac[ta] || !have_quant[comp_q[c]])
                    return;
                p.t.dc[c] = dc[td], p.t.ac[c] = ac[ta];
                std::memcpy(p.t.quant[c], quant[comp_q[c]], sizeof quant[0]);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
            {
                p.status = UNSUPPORTED;
                return;
            }
            break;
        }
        // everything else - APPn, COM - is skipped by its length
    }
    g.bpm = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    g.mw = (g.w + 8 * g.hs - 1) / (8 * g.hs), g.mh = (g.h + 8 * g.vs - 1) / (8 * g.vs);
    g.cw = (g.w + g.hs - 1) / g.hs, g.ch = (g.h + g.vs - 1) / g.vs;
    // the scan's extent: up to the first marker that is no RSTn; the restart intervals on the way
    p.scan0 = (uint32_t)at;
    const uint32_t total = p.mcus();
    uint32_t start = (uint32_t)at, mcu = 0;
    size_t i = at;
    bool more_scans = false;
    for (; i + 1 < n; i++)
    {
        if (d[i] != 0xFF || d[i + 1] == 0x00)
            continue;
        size_t j = i + 1;
        while (j < n && d[j] == 0xFF)
            j++;
        if (j >= n)
            break;
        const int m = d[j];
        if (m >= 0xD0 && m <= 0xD7)
        {
            if (g.ri == 0)
                return; // a restart marker nobody announced
            p.intervals.push_back({start, (uint32_t)i, mcu});
            mcu += (uint32_t)g.ri, start = (uint32_t)j + 1;
            i = j;
            continue;
        }
        more_scans = m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD;
        break;
    }
    const size_t scan_end = i + 1 < n ? i : n;
    p.intervals.push_back({start, (uint32_t)scan_end, mcu});
    p.scan1 = (uint32_t)scan_end;
    if (more_scans)
    {
        p.status = UNSUPPORTED;
        return;
    }
    // a block is at least two bits, a DC code and an end of block: a header that promises more blocks than the scan can
    // hold is refused here, before anything is sized from it
    uint64_t scan_bits = 0;
    for (const interval &v : p.intervals)
        scan_bits += (uint64_t)(v.byte1 - v.byte0) * 8;
    if ((uint64_t)total * (uint64_t)g.bpm * 2 > scan_bits)
        return;
    // every interval but the last holds ri MCUs, and they cover the picture
    if (g.ri > 0 ? (uint32_t)p.intervals.size() != (total + (uint32_t)g.ri - 1) / (uint32_t)g.ri : p.intervals.size() != 1)
        return;
    p.status = OK;
}

// What a caller reads of a file (ochip_jpeg_file_info of include/ochip.h, which this header does not include)
template <class Info> inline void fill_info(const parsed &p, bool apply, Info &o)
{
    const geometry &g = p.g;
    const bool swap = apply && g.orientation >= 5;
    o.width = swap ? g.h : g.w, o.height = swap ? g.w : g.h;
    o.components = g.ncomp, o.h_samp = g.hs, o.v_samp = g.vs, o.restart_interval = g.ri;
    o.orientation = g.orientation, o.status = p.status;
    o.offset = ~0ull;
}

// The first step of a decode call on either route: the arguments, every file's headers, info[] and where each image goes -
// offsets[i], or back to back in the order of the files; a file whose headers are refused takes no room.  "" or the refusal.
template <class Info>
inline std::string plan_batch(int64_t n, int64_t max_files, const uint8_t *const *files, const uint64_t *sizes, bool apply, const void *out,
                              uint64_t out_cap, const uint64_t *offsets, Info *info, std::vector<parsed> &P)
{
    if (n < 0 || n > max_files)
        return std::to_string(n) + " files, at most " + std::to_string(max_files) + " a call";
    if (n > 0 && (!files || !sizes || !info))
        return "a NULL argument";
    P.assign((size_t)n, parsed());
    uint64_t next = 0;
    for (int64_t i = 0; i < n; i++)
    {
        if (!files[i])
            return "file " + std::to_string(i) + " is NULL";
        parse(files[i], (size_t)sizes[i], P[i]);
        fill_info(P[i], apply, info[i]);
        if (P[i].status != OK)
            continue;
        const uint64_t bytes = (uint64_t)P[i].g.w * (uint64_t)P[i].g.h * 3;
        info[i].offset = offsets ? offsets[i] : next;
        next = info[i].offset + bytes;
        if (!out || info[i].offset + bytes > out_cap)
            return "image " + std::to_string(i) + " ends at byte " + std::to_string(info[i].offset + bytes) + ", the output holds " +
                   std::to_string(out ? out_cap : 0);
    }
    return "";
}

inline uint32_t interval_mcus(const parsed &p, size_t i)
{
    const uint32_t total = p.mcus(), first = p.intervals[i].first_mcu;
    return p.g.ri > 0 && first + (uint32_t)p.g.ri < total ? (uint32_t)p.g.ri : total - first;
}

} // namespace ochip_jd
