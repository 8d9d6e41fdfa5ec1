// A stand-alone program over csrc/png_rules.hpp and the host decoder (csrc/host/png_decode.hpp), built by test_png_host.py with
// -fsanitize=address,undefined: the small fixtures through the encoder and back through the decoder, byte mutations and
// truncations of a thumbnail's file, hostile headers.  Every input is a heap block of exactly its size, so a read or a write
// one byte outside it is caught.  Prints "clean" and returns 0 when every file round-trips and every damaged one is refused
// or decodes to the picture.
#include "../opencalibration_amd/csrc/host/png_decode.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace ochip_png;

namespace
{
int failures = 0;

void expect(bool ok, const char *what, long a = 0, long b = 0)
{
    if (!ok)
    {
        std::printf("FAILED: %s (%ld, %ld)\n", what, a, b);
        failures++;
    }
}

struct lcg
{
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

// a heap block of exactly n bytes
std::unique_ptr<uint8_t[]> exact(const uint8_t *src, size_t n)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n)
        std::memcpy(p.get(), src, n);
    return p;
}

// kind 0: ramp, 1: ramp plus noise of amplitude 4, 2: noise, 3: constant rows
std::vector<uint8_t> picture(uint32_t w, uint32_t h, uint32_t c, int kind, uint64_t seed)
{
    lcg r{seed};
    std::vector<uint8_t> a((size_t)w * h * c);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++)
            for (uint32_t k = 0; k < c; k++)
            {
                uint32_t v = kind == 2 ? r.next() : kind == 3 ? y * 37 : ((2 * x + 3 * y) >> k) + (kind == 1 ? r.next() % 5 : 0);
                a[((size_t)y * w + x) * c + k] = (uint8_t)v;
            }
    return a;
}

void round_trip(uint32_t w, uint32_t h, uint32_t c, int kind, bool swap, std::vector<uint8_t> *keep = nullptr)
{
    shape s;
    expect(make_shape(w, h, c, swap, s), "make_shape", w, h);
    const std::vector<uint8_t> a = picture(w, h, c, kind, 17 * w + h + c);
    const auto pix = exact(a.data(), a.size());
    std::vector<uint8_t> file, payload;
    encode_image(pix.get(), s, file, &payload);
    expect(file.size() <= file_bound(s.F), "the file's bound", (long)file.size(), (long)file_bound(s.F));
    expect(payload.size() == s.F, "the payload's size");
    const auto in = exact(file.data(), file.size());
    file_info I;
    std::vector<uint8_t> back;
    expect(decode_file(in.get(), file.size(), I, back) == PNG_OK, "decode of an encoded file", w, h);
    expect(I.width == w && I.height == h && I.channels == (int)c, "the decoded header");
    bool same = back.size() == a.size();
    for (size_t i = 0; same && i < a.size(); i++)
        same = back[i] == a[source_index((uint32_t)(i % ((size_t)w * c)), c, swap) + i / ((size_t)w * c) * ((size_t)w * c)];
    expect(same, "the decoded pixels", w, h);
    std::vector<char> text((size_t)base64_bytes(file.size()));
    base64_encode(in.get(), file.size(), text.data());
    if (keep)
        *keep = file;
}
} // namespace

int main()
{
    const uint32_t shapes[][3] = {{1, 1, 1}, {1, 1, 3}, {1, 1, 4}, {58, 43, 3}, {5, 3, 3}, {127, 128, 1}, {16384, 1, 1}, {32767, 2, 1}, {32768, 2, 1},
                                  {300, 300, 1}, {1000, 40, 1}, {61, 33, 4}};
    std::vector<uint8_t> thumb;
    for (const auto &sh : shapes)
        for (int kind = 0; kind < 4; kind++)
            for (int swap = 0; swap < 2; swap++)
                round_trip(sh[0], sh[1], sh[2], kind, swap != 0, sh[0] == 58 && kind == 1 && !swap ? &thumb : nullptr);
    // the CRC's combination against the plain CRC
    {
        const std::vector<uint8_t> a = picture(300, 50, 1, 2, 5);
        for (size_t n : {(size_t)0, (size_t)1, (size_t)4095, (size_t)4096, (size_t)4097, a.size()})
        {
            const auto p = exact(a.data(), n);
            std::vector<uint8_t> whole = {'I', 'D', 'A', 'T'};
            whole.insert(whole.end(), a.begin(), a.begin() + n);
            expect(idat_crc(p.get(), n) == crc32_of(whole.data(), whole.size()), "crc_combine", (long)n);
        }
    }
    // truncations and mutations of the noisy thumbnail's file: refused, or the picture
    file_info I;
    std::vector<uint8_t> want, got;
    expect(decode_file(thumb.data(), thumb.size(), I, want) == PNG_OK, "the thumbnail");
    for (size_t cut = 0; cut < thumb.size(); cut += cut < 64 || cut + 64 > thumb.size() ? 1 : 37)
    {
        const auto in = exact(thumb.data(), cut);
        expect(decode_file(in.get(), cut, I, got) == PNG_CORRUPT && got.empty(), "a truncated file", (long)cut);
    }
    lcg r{99};
    int refused = 0;
    for (int k = 0; k < 4000; k++)
    {
        auto in = exact(thumb.data(), thumb.size());
        in[r.next() % thumb.size()] ^= (uint8_t)(1u << (r.next() % 8));
        if (k % 4 == 0) // a second damaged byte
            in[r.next() % thumb.size()] = (uint8_t)r.next();
        const int st = decode_file(in.get(), thumb.size(), I, got);
        if (st == PNG_OK)
            expect(got == want, "a mutated file decoded to another picture", k);
        else // corrupt, never a third answer: IHDR's CRC is checked before its depth and type are looked at
            expect(st == PNG_CORRUPT && got.empty(), "a damaged file that is not corrupt, or left pixels", k), refused++;
    }
    expect(refused > 3900, "mutations refused", refused);
    // the stream alone, damaged behind valid chunk CRCs: the inflate's own bounds
    {
        const uint32_t zlen = get_be32(thumb.data() + 33);
        const uint64_t F = 43ull * (1 + 58 * 3);
        for (int k = 0; k < 4000; k++)
        {
            auto z = exact(thumb.data() + IDAT_AT, zlen);
            z[2 + r.next() % (zlen - 2)] ^= (uint8_t)(1u << (r.next() % 8));
            const size_t n = k % 8 == 0 ? r.next() % zlen : zlen;
            const auto cutz = exact(z.get(), n);
            std::vector<uint8_t> out;
            (void)inflate_exact(cutz.get(), n, F, out);
            (void)inflate_exact(cutz.get(), n, F - 1, out);
            (void)inflate_exact(cutz.get(), n, F + 1, out);
        }
    }
    // hostile headers: nothing is sized from IHDR before the data is known to be able to fill it
    for (uint32_t side : {65535u, 0x7FFFFFFFu})
    {
        std::vector<uint8_t> f(thumb);
        put_be32(f.data() + 16, side), put_be32(f.data() + 20, side);
        put_be32(f.data() + 29, crc32_of(f.data() + 12, 17));
        const auto in = exact(f.data(), f.size());
        expect(decode_file(in.get(), f.size(), I, got) == PNG_CORRUPT && got.empty(), "a hostile header", side);
    }
    expect(decode_file(nullptr, 0, I, got) == PNG_CORRUPT, "no data");
    if (failures)
        return 1;
    std::printf("clean\n");
    return 0;
}
