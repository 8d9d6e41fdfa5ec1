// A stand-alone program over csrc/deflate_rules.hpp alone (test_geotiff_host.py builds it with the system g++ under the
// address and undefined-behaviour sanitizers, host code only, a process of its own).  It drives the tile encoder to its buffer
// bounds: a noise payload (the stored form, exactly 1 048 667 bytes), a payload whose first segment has 17 values in
// Fibonacci proportion (the 15-bit limit), the payload of a 1 x 1 raster, all zeros, and the length limiter at its edges.
// Every stream is checked by a small inflate of its own for stored, fixed and dynamic blocks.
#include "../opencalibration_amd/csrc/deflate_rules.hpp"

#include <cstdio>
#include <cstdlib>

using namespace ochip_df;

namespace
{
struct bit_reader
{
    const uint8_t *p;
    size_t n, at = 0; // in bits
    uint32_t get(int k)
    {
        uint32_t v = 0;
        for (int i = 0; i < k; i++, at++)
        {
            if (at / 8 >= n)
            {
                std::printf("inflate: out of input\n");
                std::exit(1);
            }
            v |= (uint32_t)((p[at / 8] >> (at % 8)) & 1) << i;
        }
        return v;
    }
};

struct decoder
{
    int count[16] = {0}, symbol[320];
    void build(const uint8_t *lens, int n)
    {
        for (int i = 0; i < 16; i++)
            count[i] = 0;
        for (int s = 0; s < n; s++)
            count[lens[s]]++;
        int offs[16];
        offs[1] = 0;
        for (int i = 1; i < 15; i++)
            offs[i + 1] = offs[i] + count[i];
        for (int s = 0; s < n; s++)
            if (lens[s])
                symbol[offs[lens[s]]++] = s;
    }
    int decode(bit_reader &r) const
    {
        int code = 0, first = 0, index = 0;
        for (int len = 1; len <= 15; len++)
        {
            code |= (int)r.get(1);
            const int c = count[len];
            if (code - c < first)
                return symbol[index + (code - first)];
            index += c, first += c, first <<= 1, code <<= 1;
        }
        std::printf("inflate: bad code\n");
        std::exit(1);
    }
};

std::vector<uint8_t> inflate(const std::vector<uint8_t> &z)
{
    static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const int dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    std::vector<uint8_t> out;
    if (z.size() < 6 || z[0] != 0x78 || z[1] != 0x9C)
    {
        std::printf("inflate: no zlib header\n");
        std::exit(1);
    }
    bit_reader r{z.data() + 2, z.size() - 6};
    for (int final = 0; !final;)
    {
        final = (int)r.get(1);
        const int type = (int)r.get(2);
        if (type == 0)
        {
            r.at = (r.at + 7) / 8 * 8;
            const uint32_t len = r.get(16), nlen = r.get(16);
            if ((len ^ nlen) != 0xFFFF)
                std::printf("inflate: stored lengths\n"), std::exit(1);
            for (uint32_t i = 0; i < len; i++)
                out.push_back((uint8_t)r.get(8));
            continue;
        }
        uint8_t lens[320] = {0};
        decoder lit, dist;
        if (type == 1)
        {
            for (int s = 0; s < 288; s++)
                lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            lit.build(lens, 288);
            for (int s = 0; s < 30; s++)
                lens[s] = 5;
            dist.build(lens, 30);
        }
        else if (type == 2)
        {
            const int hlit = (int)r.get(5) + 257, hdist = (int)r.get(5) + 1, hclen = (int)r.get(4) + 4;
            uint8_t cl[19] = {0};
            for (int i = 0; i < hclen; i++)
                cl[order[i]] = (uint8_t)r.get(3);
            decoder cld;
            cld.build(cl, 19);
            for (int i = 0; i < hlit + hdist;)
            {
                const int s = cld.decode(r);
                if (s < 16)
                    lens[i++] = (uint8_t)s;
                else
                {
                    const int rep = s == 16 ? 3 + (int)r.get(2) : s == 17 ? 3 + (int)r.get(3) : 11 + (int)r.get(7);
                    const uint8_t v = s == 16 ? lens[i - 1] : 0;
                    if ((s == 16 && i == 0) || i + rep > hlit + hdist)
                        std::printf("inflate: bad repeat\n"), std::exit(1);
                    for (int k = 0; k < rep; k++)
                        lens[i++] = v;
                }
            }
            if (lens[256] == 0)
                std::printf("inflate: no end of block\n"), std::exit(1);
            lit.build(lens, hlit);
            dist.build(lens + hlit, hdist);
        }
        else
            std::printf("inflate: block type 3\n"), std::exit(1);
        for (;;)
        {
            const int s = lit.decode(r);
            if (s == 256)
                break;
            if (s < 256)
            {
                out.push_back((uint8_t)s);
                continue;
            }
            const int len = lbase[s - 257] + (int)r.get(lext[s - 257]);
            const int ds = dist.decode(r);
            const size_t d = (size_t)dbase[ds] + r.get(dext[ds]);
            if (d > out.size())
                std::printf("inflate: distance %zu at %zu\n", d, out.size()), std::exit(1);
            for (int k = 0; k < len; k++)
                out.push_back(out[out.size() - d]);
        }
    }
    const uint32_t want = (uint32_t)z[z.size() - 4] << 24 | (uint32_t)z[z.size() - 3] << 16 | (uint32_t)z[z.size() - 2] << 8 | z[z.size() - 1];
    if (want != adler32(out.data(), out.size()))
        std::printf("inflate: Adler-32\n"), std::exit(1);
    return out;
}

uint32_t rng_state = 12345;
uint32_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
    return rng_state;
}

size_t round_trip(const char *what, const std::vector<uint8_t> &payload)
{
    // exactly sized: a byte beyond either end is the sanitizer's
    std::vector<uint8_t> exact(payload.begin(), payload.end()), z;
    encode_tile(exact.data(), z);
    if (z.size() > (size_t)STORED_BYTES || inflate(z) != payload)
    {
        std::printf("%s: %zu bytes do not inflate to the payload\n", what, z.size());
        std::exit(1);
    }
    std::printf("%s: %zu bytes\n", what, z.size());
    return z.size();
}

void limiter(const char *what, const std::vector<uint32_t> &counts, int limit)
{
    std::vector<uint8_t> lens(counts.size());
    block_work W;
    code_lengths(counts.data(), (int)counts.size(), limit, lens.data(), W.key, W.sym, W.num);
    uint64_t kraft = 0;
    int used = 0;
    for (size_t s = 0; s < counts.size(); s++)
    {
        if ((counts[s] == 0) != (lens[s] == 0) || lens[s] > limit)
            std::printf("%s: symbol %zu has length %d\n", what, s, lens[s]), std::exit(1);
        if (lens[s])
            kraft += 1ull << (limit - lens[s]), used++;
    }
    if (kraft > (1ull << limit) || (used >= 2 && kraft != (1ull << limit)))
        std::printf("%s: Kraft sum %llu of %llu\n", what, (unsigned long long)kraft, 1ull << limit), std::exit(1);
}
} // namespace

int main()
{
    std::vector<uint8_t> p(PAYLOAD);
    for (auto &b : p)
        b = (uint8_t)(rnd() >> 11);
    if (round_trip("noise", p) != (size_t)STORED_BYTES)
        return std::printf("noise is not stored\n"), 1;
    std::fill(p.begin(), p.end(), 0);
    round_trip("zeros", p);
    p[0] = 9, p[1] = 8, p[2] = 7, p[3] = 255; // a 1 x 1 raster's tile
    round_trip("one pixel", p);
    {
        std::fill(p.begin(), p.end(), 0);
        uint32_t fib[17] = {1, 1}, at = 0;
        for (int i = 2; i < 17; i++)
            fib[i] = fib[i - 1] + fib[i - 2];
        std::vector<uint8_t> bytes;
        for (int i = 0; i < 17; i++)
            for (uint32_t k = 0; k < fib[i]; k++)
                bytes.push_back((uint8_t)(i + 1));
        for (size_t i = bytes.size(); i > 1; i--)
            std::swap(bytes[i - 1], bytes[rnd() % i]);
        for (uint8_t b : bytes)
            p[at++] = b;
        for (size_t i = SEGMENT; i < p.size(); i++)
            p[i] = (uint8_t)((((i >> 2) * 7 + (i & 3) * 3 + (i >> 11) * 5)) & 63);
        round_trip("fibonacci", p);
    }
    {
        std::vector<uint32_t> c = {1, 1};
        while (c.size() < 40)
            c.push_back(c[c.size() - 1] + c[c.size() - 2]);
        limiter("fibonacci, 15 bits", c, 15);
        c.resize(19);
        limiter("fibonacci, 7 bits", c, 7);
        limiter("equal", std::vector<uint32_t>(286, 5), 15);
        limiter("equal, 9 bits", std::vector<uint32_t>(286, 5), 9);
        limiter("one", {0, 0, 3, 0}, 15);
        limiter("two", {0, 4, 3, 0}, 15);
        limiter("none", {0, 0, 0, 0}, 15);
    }
    std::printf("ok\n");
    return 0;
}
