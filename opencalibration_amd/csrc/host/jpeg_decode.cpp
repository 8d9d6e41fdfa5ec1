// liboc_host.so: baseline JPEG decoding of the load stage (csrc/jpeg_decode.hpp; the reference's
// cv::imread(path), src/extract/extract_image.cpp:18-21).  The CPU route - the shared header's rules in straight loops, one
// symbol after the other, OpenMP over the images of a batch - and the C ABI over both routes.  The CPU route is the
// yardstick of the device route's tests.  With OCHIP_JPEG_DECODE_STANDALONE defined the device route is left out and the
// file links without libochip.so: tests/jpeg_decode_driver.cpp builds from it that way.
#include "../../../include/oc_host.h"

#include "../jpeg_decode.hpp"
#include "../live_handles.hpp"

#include <memory>
#include <string>
#include <vector>

namespace
{
using namespace ochip_jd;

thread_local std::string decode_error;

int fail(const std::string &text)
{
    decode_error = text;
    return -1;
}

ochip::live_set<och_jpeg_decoder> g_live; // the decoders that exist

// The coefficients of every block, natural order, in the scan's order; false: the scan is not decodable
bool decode_scan(const uint8_t *d, const parsed &p, std::vector<int16_t> &coef)
{
    const geometry &g = p.g;
    coef.assign((size_t)p.mcus() * (size_t)g.bpm * 64, 0);
    for (size_t i = 0; i < p.intervals.size(); i++)
    {
        const interval &iv = p.intervals[i];
        const bit_reader r{d, iv.byte1};
        const uint32_t end_bit = iv.byte1 * 8u;
        uint32_t cur = iv.first_mcu * (uint32_t)g.bpm;
        const uint32_t block_end = cur + interval_mcus(p, i) * (uint32_t)g.bpm;
        walk_state s{iv.byte0 * 8u, 0, 0};
        int pred[3] = {0, 0, 0};
        while (cur < block_end)
        {
            if (s.pos >= end_bit)
                return false;
            const int c = component_of_block(g, s.blk);
            const symbol y = next_symbol(r, p.t, g, s, end_bit);
            if (y.bad)
                return false;
            if (y.zz == 0)
            {
                pred[c] += y.value;
                coef[(size_t)cur * 64] = (int16_t)pred[c];
            }
            else if (y.zz > 0)
                coef[(size_t)cur * 64 + ZIGZAG[y.zz]] = (int16_t)y.value;
            if (y.block_done)
                cur++;
        }
    }
    return true;
}

// One file into out (h x w x 3, oriented when apply); the status
int32_t decode_file(const uint8_t *d, const parsed &p, bool apply, uint8_t *out)
{
    const geometry &g = p.g;
    std::vector<int16_t> coef;
    if (!decode_scan(d, p, coef))
        return CORRUPT;
    std::vector<uint8_t> plane[3];
    int stride[3];
    for (int c = 0; c < g.ncomp; c++)
    {
        stride[c] = c == 0 ? g.yw() : g.pcw();
        plane[c].resize((size_t)stride[c] * (size_t)(c == 0 ? g.yh() : g.pch()));
    }
    const uint32_t blocks = p.mcus() * (uint32_t)g.bpm;
    for (uint32_t n = 0; n < blocks; n++)
    {
        int c, bx, by;
        place_block(g, n, c, bx, by);
        idct_block(coef.data() + (size_t)n * 64, p.t.quant[c], plane[c].data() + (size_t)by * 8 * stride[c] + (size_t)bx * 8, stride[c]);
    }
    const int o = apply ? g.orientation : 1, ow = oriented_width(o, g.w, g.h);
    for (int y = 0; y < g.h; y++)
        for (int x = 0; x < g.w; x++)
        {
            int ox, oy;
            oriented(o, g.w, g.h, x, y, ox, oy);
            uint8_t *px = out + ((size_t)oy * (size_t)ow + (size_t)ox) * 3;
            const int Y = plane[0][(size_t)y * stride[0] + x];
            if (g.ncomp == 1)
                px[0] = px[1] = px[2] = (uint8_t)Y;
            else
                ycc_to_bgr(Y, chroma_at(plane[1].data(), stride[1], g, x, y), chroma_at(plane[2].data(), stride[2], g, x, y), px);
        }
    return OK;
}
} // namespace

struct och_jpeg_decoder
{
    ochip_ctx *ctx = nullptr;
    ochip_jpeg_decoder *dev = nullptr;
};

extern "C"
{

const char *och_jpeg_decode_last_error(void)
{
    return decode_error.c_str();
}

int och_jpeg_info(const uint8_t *data, uint64_t size, int apply_orientation, ochip_jpeg_file_info *out)
{
    if (!data || !out)
        return fail("och_jpeg_info: a NULL argument");
    parsed p;
    parse(data, (size_t)size, p);
    fill_info(p, apply_orientation != 0, *out);
    return 0;
}

int och_jpeg_decoder_create(ochip_ctx *ctx, int subsequence_bits, och_jpeg_decoder **out)
{
    if (!out)
        return fail("och_jpeg_decoder_create: out is NULL");
    *out = nullptr;
    if (subsequence_bits != 0 && (subsequence_bits < MIN_SUBSEQUENCE_BITS || subsequence_bits % 32 != 0))
        return fail("och_jpeg_decoder_create: subsequence_bits " + std::to_string(subsequence_bits) + " is neither 0 nor a multiple of 32 from " +
                    std::to_string(MIN_SUBSEQUENCE_BITS) + " on");
    std::unique_ptr<och_jpeg_decoder> d(new och_jpeg_decoder);
    d->ctx = ctx;
    if (ctx)
    {
#ifdef OCHIP_JPEG_DECODE_STANDALONE
        return fail("och_jpeg_decoder_create: built without the device route");
#else
        if (ochip_jpeg_decoder_create(ctx, subsequence_bits, &d->dev) != OCHIP_OK)
            return fail(ochip_last_error(ctx));
#endif
    }
    g_live.add(d.get());
    *out = d.release();
    return 0;
}

int och_jpeg_decoder_decode(och_jpeg_decoder *d, int64_t n, const uint8_t *const *files, const uint64_t *sizes, int apply_orientation,
                            void *out, uint64_t out_cap, const uint64_t *offsets, ochip_jpeg_file_info *info, int32_t *rounds)
{
    if (!g_live.has(d))
        return fail("och_jpeg_decoder_decode: not a live och_jpeg_decoder object");
#ifndef OCHIP_JPEG_DECODE_STANDALONE
    if (d->dev)
        return ochip_jpeg_decoder_decode(d->dev, n, files, sizes, apply_orientation, out, out_cap, offsets, info, rounds) == OCHIP_OK
                   ? 0
                   : fail(ochip_last_error(d->ctx));
#endif
    std::vector<parsed> P;
    const std::string refusal = plan_batch(n, MAX_BATCH_FILES, files, sizes, apply_orientation != 0, out, out_cap, offsets, info, P);
    if (!refusal.empty())
        return fail("och_jpeg_decoder_decode: " + refusal);
    if (rounds)
        rounds[0] = rounds[1] = 0;
    const bool apply = apply_orientation != 0;
#pragma omp parallel for schedule(dynamic)
    for (int64_t i = 0; i < n; i++)
        if (P[i].status == OK)
            info[i].status = decode_file(files[i], P[i], apply, static_cast<uint8_t *>(out) + info[i].offset);
    return 0;
}

void och_jpeg_decoder_destroy(och_jpeg_decoder *d)
{
    if (!g_live.remove(d))
        return;
#ifndef OCHIP_JPEG_DECODE_STANDALONE
    ochip_jpeg_decoder_destroy(d->dev);
#endif
    delete d;
}

} // extern "C"
