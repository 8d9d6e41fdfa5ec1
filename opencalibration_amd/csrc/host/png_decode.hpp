// The PNG decoder of the host library (the reference's cv::imdecode of a node's thumbnail,
// src/io/deserialize_MeasurementGraph.cpp:73-80).  Host code only: a thumbnail is a few kilobytes of strictly sequential
// inflate.  Plain C++ over csrc/png_rules.hpp, so a stand-alone program builds from it.  Taken: 8-bit colour types 0, 2, 4
// and 6, non-interlaced, any number of IDAT chunks, ancillary chunks skipped.  Everything is checked - the signature, every
// chunk's CRC, the zlib header, the Huffman codes, the distances, the Adler-32, the inflated size against IHDR, the filter
// types - and a file that fails a check gives no picture at all.  Writes are bounded by h * stride from IHDR, reads by the
// data's end, and nothing is sized from IHDR before the data is known to be able to fill it.
#pragma once

#include "../png_rules.hpp"

#include <cstdlib>
#include <vector>

namespace ochip_png
{

constexpr int PNG_OK = 0, PNG_UNSUPPORTED = 1, PNG_CORRUPT = 2;

struct file_info
{
    uint32_t width = 0, height = 0;
    int32_t bit_depth = 0, color_type = 0, interlace = 0, channels = 0, status = PNG_CORRUPT;
};

inline uint32_t get_be32(const uint8_t *p)
{
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// Signature and IHDR alone
inline int read_info(const uint8_t *data, uint64_t size, file_info &I)
{
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    I = file_info();
    if (!data || size < 33 || std::memcmp(data, sig, 8) != 0)
        return I.status = PNG_CORRUPT;
    if (get_be32(data + 8) != 13 || std::memcmp(data + 12, "IHDR", 4) != 0 || crc32_of(data + 12, 17) != get_be32(data + 29))
        return I.status = PNG_CORRUPT;
    I.width = get_be32(data + 16), I.height = get_be32(data + 20);
    I.bit_depth = data[24], I.color_type = data[25], I.interlace = data[28];
    if (I.width == 0 || I.height == 0 || I.width > 0x7FFFFFFFu || I.height > 0x7FFFFFFFu || data[26] != 0 || data[27] != 0 || I.interlace > 1)
        return I.status = PNG_CORRUPT;
    const int d = I.bit_depth, t = I.color_type;
    const bool depth_ok = t == 0   ? (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)
                          : t == 3 ? (d == 1 || d == 2 || d == 4 || d == 8)
                                   : (t == 2 || t == 4 || t == 6) && (d == 8 || d == 16);
    if (!depth_ok)
        return I.status = PNG_CORRUPT;
    I.channels = t == 0 ? 1 : t == 2 ? 3 : t == 3 ? 1 : t == 4 ? 2 : 4;
    if (t == 3 || d != 8 || I.interlace != 0)
        return I.status = PNG_UNSUPPORTED;
    return I.status = PNG_OK;
}

namespace inflate_detail
{
struct bits_in
{
    const uint8_t *p;
    size_t n, at = 0;
    uint64_t acc = 0;
    int cnt = 0;
    bool fail = false;
    uint32_t take(int k) // k <= 16
    {
        while (cnt < k)
        {
            if (at >= n)
            {
                fail = true;
                return 0;
            }
            acc |= (uint64_t)p[at++] << cnt, cnt += 8;
        }
        const uint32_t v = (uint32_t)(acc & ((1u << k) - 1));
        acc >>= k, cnt -= k;
        return v;
    }
    void align()
    {
        acc >>= cnt & 7, cnt -= cnt & 7;
    }
};

struct huffman
{
    uint16_t count[16];
    uint16_t symbol[288];
};

// false: over-subscribed, or incomplete in a way inflate refuses (more than a single code of one bit; never for the
// code-length code)
inline bool build(huffman &h, const uint8_t *lens, int n, bool may_be_single)
{
    for (int i = 0; i < 16; i++)
        h.count[i] = 0;
    for (int i = 0; i < n; i++)
        h.count[lens[i]]++;
    int left = 1, longest = 0;
    for (int l = 1; l < 16; l++)
    {
        left <<= 1, left -= h.count[l];
        if (left < 0)
            return false;
        if (h.count[l])
            longest = l;
    }
    if (left > 0 && longest != 0 && !(may_be_single && longest == 1))
        return false;
    if (longest == 0 && !may_be_single)
        return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; l++)
        offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int i = 0; i < n; i++)
        if (lens[i])
            h.symbol[offs[lens[i]]++] = (uint16_t)i;
    return true;
}

inline int decode(bits_in &in, const huffman &h) // -1: no such code, or the data ended
{
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++)
    {
        code |= (int)in.take(1);
        if (in.fail)
            return -1;
        const int count = h.count[l];
        if (code - count < first)
            return h.symbol[index + (code - first)];
        index += count, first += count, first <<= 1, code <<= 1;
    }
    return -1;
}
} // namespace inflate_detail

// A zlib stream of exactly `expect` bytes into out (sized here, once the stream is known to be able to fill it).  false: any
// check fails, the stream gives fewer or more bytes, or bytes follow its Adler-32.
inline bool inflate_exact(const uint8_t *z, size_t n, uint64_t expect, std::vector<uint8_t> &out)
{
    using namespace inflate_detail;
    // deflate expands at most 1032 : 1 (258 bytes from a two-bit pair of codes)
    if (n < 6 || expect > (uint64_t)n * 1032 || expect > ((uint64_t)1 << 40))
        return false;
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || ((uint32_t)z[0] << 8 | z[1]) % 31 != 0 || (z[1] & 0x20))
        return false;
    out.clear();
    out.resize((size_t)expect);
    uint8_t *o = out.data();
    uint64_t have = 0;
    bits_in in{z + 2, n - 2};
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    huffman lit, dist;
    uint8_t lens[320];
    for (bool last = false; !last;)
    {
        last = in.take(1) != 0;
        const uint32_t type = in.take(2);
        if (in.fail || type == 3)
            return false;
        if (type == 0)
        {
            in.align();
            const uint32_t len = in.take(16), nlen = in.take(16);
            if (in.fail || (len ^ 0xFFFFu) != nlen || have + len > expect)
                return false;
            for (uint32_t i = 0; i < len; i++) // the bit buffer holds whole bytes here
            {
                o[have++] = (uint8_t)in.take(8);
                if (in.fail)
                    return false;
            }
            continue;
        }
        if (type == 1)
        {
            for (int i = 0; i < 288; i++)
                lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            build(lit, lens, 288, false);
            for (int i = 0; i < 32; i++) // 30 and 31 complete the code and are refused where they occur
                lens[i] = 5;
            build(dist, lens, 32, true);
        }
        else
        {
            const int hlit = (int)in.take(5) + 257, hdist = (int)in.take(5) + 1, hclen = (int)in.take(4) + 4;
            if (in.fail || hlit > 286 || hdist > 30)
                return false;
            uint8_t cl[19] = {0};
            for (int i = 0; i < hclen; i++)
                cl[order[i]] = (uint8_t)in.take(3);
            if (in.fail)
                return false;
            huffman clh;
            if (!build(clh, cl, 19, false))
                return false;
            for (int i = 0; i < hlit + hdist;)
            {
                const int s = decode(in, clh);
                if (s < 0)
                    return false;
                if (s < 16)
                {
                    lens[i++] = (uint8_t)s;
                    continue;
                }
                int rep, val = 0;
                if (s == 16)
                {
                    if (i == 0)
                        return false;
                    val = lens[i - 1], rep = 3 + (int)in.take(2);
                }
                else
                    rep = s == 17 ? 3 + (int)in.take(3) : 11 + (int)in.take(7);
                if (in.fail || i + rep > hlit + hdist)
                    return false;
                while (rep--)
                    lens[i++] = (uint8_t)val;
            }
            if (lens[256] == 0)
                return false; // no end-of-block code
            uint8_t dl[30];
            for (int i = 0; i < hdist; i++)
                dl[i] = lens[hlit + i];
            if (!build(lit, lens, hlit, true) || !build(dist, dl, hdist, true))
                return false;
        }
        for (;;)
        {
            const int s = decode(in, lit);
            if (s < 0)
                return false;
            if (s < 256)
            {
                if (have >= expect)
                    return false;
                o[have++] = (uint8_t)s;
                continue;
            }
            if (s == 256)
                break;
            if (s > 285)
                return false;
            const uint32_t len = len_base[s - 257] + in.take(len_extra[s - 257]);
            const int ds = decode(in, dist);
            if (ds < 0 || ds > 29)
                return false;
            const uint32_t d = dist_base[ds] + in.take(dist_extra[ds]);
            if (in.fail || d > have || have + len > expect)
                return false;
            for (uint32_t i = 0; i < len; i++, have++)
                o[have] = o[have - d];
        }
    }
    if (have != expect)
        return false;
    in.align();
    uint32_t adler = 0;
    for (int i = 0; i < 4; i++)
        adler = adler << 8 | in.take(8);
    if (in.fail || in.cnt != 0 || in.at != in.n) // bytes behind the Adler-32: trailing garbage inside the stream
        return false;
    return adler == adler32(o, (size_t)expect);
}

// The picture of a file: width x height x channels bytes, the file's channels.  PNG_OK only with every check passed; pixels
// is empty otherwise.
inline int decode_file(const uint8_t *data, uint64_t size, file_info &I, std::vector<uint8_t> &pixels)
{
    pixels.clear();
    if (read_info(data, size, I) != PNG_OK)
        return I.status;
    // the chunks: every CRC checked, IDATs consecutive and concatenated, ancillary ones skipped, IEND last and the file's end
    std::vector<uint8_t> z;
    uint64_t at = 33;
    bool seen_idat = false, idat_over = false, ended = false;
    while (!ended)
    {
        if (size - at < 12)
            return I.status = PNG_CORRUPT;
        const uint64_t len = get_be32(data + at);
        if (len > 0x7FFFFFFFu || size - at - 12 < len)
            return I.status = PNG_CORRUPT;
        const uint8_t *type = data + at + 4, *body = type + 4;
        if (crc32_of(type, (size_t)len + 4) != get_be32(body + len))
            return I.status = PNG_CORRUPT;
        for (int i = 0; i < 4; i++)
            if (!((type[i] >= 'A' && type[i] <= 'Z') || (type[i] >= 'a' && type[i] <= 'z')))
                return I.status = PNG_CORRUPT;
        const bool idat = std::memcmp(type, "IDAT", 4) == 0;
        if (idat)
        {
            if (idat_over)
                return I.status = PNG_CORRUPT;
            seen_idat = true;
            z.insert(z.end(), body, body + len);
        }
        else
        {
            idat_over = seen_idat;
            if (std::memcmp(type, "IEND", 4) == 0)
            {
                if (len != 0)
                    return I.status = PNG_CORRUPT;
                ended = true;
            }
            else if (std::memcmp(type, "IHDR", 4) == 0)
                return I.status = PNG_CORRUPT;
            else if (std::memcmp(type, "PLTE", 4) == 0)
            {
                if (seen_idat || I.color_type == 0 || I.color_type == 4 || len % 3 != 0)
                    return I.status = PNG_CORRUPT;
            }
            else if (!(type[0] & 0x20)) // a critical chunk this decoder does not know
                return I.status = PNG_CORRUPT;
        }
        at += 12 + len;
    }
    if (at != size || !seen_idat)
        return I.status = PNG_CORRUPT;
    const uint64_t c = (uint64_t)I.channels, stride = 1 + (uint64_t)I.width * c, F = (uint64_t)I.height * stride;
    std::vector<uint8_t> payload;
    if (!inflate_exact(z.data(), z.size(), F, payload))
        return I.status = PNG_CORRUPT;
    for (uint64_t y = 0; y < I.height; y++)
        if (payload[(size_t)(y * stride)] > 4)
            return I.status = PNG_CORRUPT;
    const uint64_t n = (uint64_t)I.width * c;
    pixels.resize((size_t)(I.height * n));
    for (uint64_t y = 0; y < I.height; y++)
    {
        const uint8_t *row = payload.data() + (size_t)(y * stride);
        uint8_t *cur = pixels.data() + (size_t)(y * n);
        const uint8_t *above = y ? cur - n : nullptr;
        const int type = row[0];
        for (uint64_t x = 0; x < n; x++)
        {
            const int a = x >= c ? cur[x - c] : 0, b = above ? above[x] : 0, cc = above && x >= c ? above[x - c] : 0;
            const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, cc);
            cur[x] = (uint8_t)(row[1 + x] + pred);
        }
    }
    return I.status = PNG_OK;
}

// The picture as three channels, the way cv::imdecode's IMREAD_COLOR gives it but for the order (the file's R G B): gray
// replicated, alpha dropped
inline void to_three_channels(const std::vector<uint8_t> &pixels, const file_info &I, std::vector<uint8_t> &rgb)
{
    const size_t count = (size_t)I.width * I.height, c = (size_t)I.channels;
    rgb.resize(count * 3);
    for (size_t i = 0; i < count; i++)
        for (size_t k = 0; k < 3; k++)
            rgb[3 * i + k] = pixels[c * i + (c >= 3 ? k : 0)];
}

} // namespace ochip_png
