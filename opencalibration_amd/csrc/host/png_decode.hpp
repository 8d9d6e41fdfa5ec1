// The PNG decoder of the host library (the reference's cv::imdecode of a node's thumbnail,
// src/io/deserialize_MeasurementGraph.cpp:73-80).  Host code only: a thumbnail is a few kilobytes of strictly sequential
// inflate.  Plain C++ over csrc/png_rules.hpp, so a stand-alone program builds from it.  Taken: 8-bit colour types 0, 2, 4
// and 6, non-interlaced, any number of IDAT chunks, ancillary chunks skipped.  Everything is checked - the signature, every
// chunk's CRC, the zlib header, the Huffman codes, the distances, the Adler-32, the inflated size against IHDR, the filter
// types - and a file that fails a check gives no picture at all.  Writes are bounded by h * stride from IHDR, reads by the
// data's end, and nothing is sized from IHDR before the data is known to be able to fill it.
#pragma once

#include "../inflate_rules.hpp"
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

// A zlib stream of exactly `expect` bytes into out (sized here, once the stream is known to be able to fill it).  false: any
// check of the project's one inflate (csrc/inflate_rules.hpp) fails, the stream gives fewer or more bytes, or bytes follow
// its Adler-32.
inline bool inflate_exact(const uint8_t *z, size_t n, uint64_t expect, std::vector<uint8_t> &out)
{
    if (!ochip_inf::plausible(n, expect))
        return false;
    out.clear();
    out.resize((size_t)expect);
    return ochip_inf::inflate_stream(z, n, out.data(), expect).status == ochip_inf::INF_OK;
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
