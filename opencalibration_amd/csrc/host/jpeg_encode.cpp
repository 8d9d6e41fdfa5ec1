// liboc_host.so: the textured OBJ's JPEG texture (csrc/jpeg_encode.hpp; the reference's
// cv::imwrite(jpg_path, texture), src/ortho/ortho.cpp:2096-2123).  The CPU route - the shared header's rules in straight
// loops, the coefficients under OpenMP over the MCUs, the entropy coder serially - and the C ABI over both routes.  The CPU
// route never hands a raster to the device by size: it is the yardstick of the device route's tests.
#include "../../../include/oc_host.h"

#include "../jpeg_encode.hpp"
#include "../live_handles.hpp"

#include <memory>
#include <string>
#include <vector>

namespace
{
using namespace ochip_jp;

thread_local std::string jpeg_error;

int fail(int code, const std::string &text)
{
    jpeg_error = text;
    return code;
}

ochip::live_set<och_jpeg> g_live; // the encoders that exist

// Whole bytes go to the stream with an FF followed by 00; the bits of the last partial byte stay in acc
struct byte_writer
{
    std::vector<uint8_t> &out;
    uint64_t acc;
    int n;
    void put(uint32_t bits, int len)
    {
        acc = (acc << len) | bits, n += len;
        while (n >= 8)
        {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            out.push_back(b);
            if (b == 0xFF)
                out.push_back(0);
            n -= 8;
        }
        acc &= (1ull << n) - 1;
    }
};

// The 384 quantised coefficients of the MCU at (mx, my) in zigzag order: Y00 Y01 Y10 Y11 Cb Cr
void mcu_coefficients(const rows_view &v, const geometry &g, const tables &t, int mx, int my, int16_t *out)
{
    for (int b = 0; b < MCU_BLOCKS; b++)
    {
        int16_t *zz = out + b * 64;
        if (b < 4 && !luma_block_real(g, mx, my, b))
        {
            for (int k = 0; k < 64; k++)
                zz[k] = 0;
            zz[0] = zz[-64]; // the block coded before it in this MCU (block 0 always exists)
            continue;
        }
        int blk[64];
        for (int r = 0; r < 8; r++)
        {
            int d[8];
            for (int c = 0; c < 8; c++)
            {
                if (b < 4)
                    d[c] = luma_sample(v, g, (int64_t)mx * 16 + (b & 1) * 8 + c, (int64_t)my * 16 + (b >> 1) * 8 + r) - 128;
                else
                {
                    int cb, cr;
                    chroma_sample(v, g, (int64_t)mx * 8 + c, (int64_t)my * 8 + r, cb, cr);
                    d[c] = (b == 4 ? cb : cr) - 128;
                }
            }
            fdct8<true>(d);
            for (int c = 0; c < 8; c++)
                blk[r * 8 + c] = d[c];
        }
        for (int c = 0; c < 8; c++)
        {
            int d[8];
            for (int r = 0; r < 8; r++)
                d[r] = blk[r * 8 + c];
            fdct8<false>(d);
            for (int r = 0; r < 8; r++)
                blk[r * 8 + c] = d[r];
        }
        const uint16_t *q = t.qdiv[b < 4 ? 0 : 1];
        for (int k = 0; k < 64; k++)
            zz[k] = (int16_t)quantise(blk[t.zz[k]], q[t.zz[k]]);
    }
}
} // namespace

struct och_jpeg
{
    ochip_ctx *ctx = nullptr;
    ochip_jpeg *dev = nullptr; // the device route
    // the CPU route
    geometry g;
    tables t;
    progress P;
    byte_stream out;
    std::vector<uint8_t> carry; // [15][w][3]
    int pred[3] = {0, 0, 0};
    uint64_t acc = 0;
    int nbits = 0;
};

namespace
{
void encode_rows(och_jpeg *e, const rows_view &v, int64_t mcu_row0, int64_t mcu_rows)
{
    const int64_t mw = e->g.mw, n = mcu_rows * mw;
    std::vector<int16_t> coef((size_t)n * MCU_COEFS);
#pragma omp parallel for schedule(static)
    for (int64_t m = 0; m < n; m++)
        mcu_coefficients(v, e->g, e->t, (int)(m % mw), (int)(mcu_row0 + m / mw), coef.data() + (size_t)m * MCU_COEFS);
    byte_writer w{e->out.bytes, e->acc, e->nbits};
    for (int64_t m = 0; m < n; m++)
        for (int b = 0; b < MCU_BLOCKS; b++)
        {
            const int16_t *zz = coef.data() + (size_t)m * MCU_COEFS + b * 64;
            const int c = b < 4 ? 0 : b - 3;
            block_coder<byte_writer> coder(w, e->t.dc[c ? 1 : 0], e->t.ac[c ? 1 : 0]);
            coder.dc(zz[0] - e->pred[c]);
            e->pred[c] = zz[0];
            for (int k = 1; k < 64; k++)
                coder.ac(zz[k]);
            coder.end();
        }
    e->acc = w.acc, e->nbits = w.n;
}
} // namespace

extern "C"
{

const char *och_jpeg_last_error(void)
{
    return jpeg_error.c_str();
}

int och_jpeg_create(ochip_ctx *ctx, int64_t width, int64_t height, int quality, och_jpeg **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_jpeg_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_jpeg> e(new och_jpeg);
    e->ctx = ctx;
    if (ctx)
    {
        const int rc = ochip_jpeg_create(ctx, width, height, quality, &e->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
    }
    else
    {
        const std::string refusal = refuse_create(width, height, quality);
        if (!refusal.empty())
            return fail(OCHIP_EINVAL, "och_jpeg_create: " + refusal);
        e->g = make_geometry(width, height);
        build_tables(quality, e->t);
        e->P.height = height;
        e->carry.resize((size_t)15 * (size_t)width * 3);
        append_header(e->out.bytes, e->g, e->t);
    }
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

int och_jpeg_feed(och_jpeg *e, int64_t row0, int64_t rows, const void *pixels, int pixel_stride, int on_device)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_jpeg_feed: not a live och_jpeg object");
    if (e->dev)
    {
        const int rc = ochip_jpeg_feed(e->dev, row0, rows, pixels, pixel_stride, on_device);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    if (!pixels)
        return fail(OCHIP_EINVAL, "och_jpeg_feed: the band is NULL");
    if (pixel_stride != 3 && pixel_stride != 4)
        return fail(OCHIP_EINVAL, "och_jpeg_feed: a pixel of " + std::to_string(pixel_stride) + " bytes, it has 3 or 4");
    if (on_device)
        return fail(OCHIP_EINVAL, "och_jpeg_feed: a band on the device needs a device context");
    progress::plan p;
    const bool was_finished = e->P.finished;
    const std::string refusal = e->P.feed(row0, rows, p);
    if (!refusal.empty())
        return fail(was_finished ? OCHIP_ESTATE : OCHIP_EINVAL, "och_jpeg_feed: " + refusal);
    const uint8_t *band = static_cast<const uint8_t *>(pixels);
    const size_t w = (size_t)e->g.w;
    if (p.mcu_rows > 0)
    {
        rows_view v;
        v.carry = e->carry.data(), v.carry_row0 = p.mcu_row0 * 16, v.carry_stride = 3;
        v.band = band, v.band_row0 = row0, v.band_stride = pixel_stride, v.w = e->g.w;
        encode_rows(e, v, p.mcu_row0, p.mcu_rows);
    }
    for (int64_t r = 0; r < p.keep_rows; r++)
    {
        const uint8_t *src = band + (size_t)(p.keep_from + r - row0) * w * (size_t)pixel_stride;
        uint8_t *dst = e->carry.data() + (size_t)(p.keep_at + r) * w * 3;
        for (size_t x = 0; x < w; x++)
            for (int c = 0; c < 3; c++)
                dst[3 * x + c] = src[(size_t)pixel_stride * x + c];
    }
    return OCHIP_OK;
}

int64_t och_jpeg_pending(och_jpeg *e)
{
    if (!g_live.has(e))
        return 0;
    return e->dev ? ochip_jpeg_pending(e->dev) : (int64_t)e->out.bytes.size();
}

int och_jpeg_collect(och_jpeg *e, uint8_t *buf, uint64_t cap, uint64_t *n)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_jpeg_collect: not a live och_jpeg object");
    if (!n)
        return fail(OCHIP_EINVAL, "och_jpeg_collect: no count");
    if (e->dev)
    {
        const int rc = ochip_jpeg_collect(e->dev, buf, cap, n);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    const std::string refusal = e->out.collect(buf, cap, n);
    return refusal.empty() ? OCHIP_OK : fail(OCHIP_EINVAL, "och_jpeg_collect: " + refusal);
}

int och_jpeg_finish(och_jpeg *e)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_jpeg_finish: not a live och_jpeg object");
    if (e->dev)
    {
        const int rc = ochip_jpeg_finish(e->dev);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    const std::string refusal = e->P.finish();
    if (!refusal.empty())
        return fail(OCHIP_ESTATE, "och_jpeg_finish: " + refusal);
    append_tail(e->out.bytes, (uint32_t)e->acc, e->nbits);
    return OCHIP_OK;
}

void och_jpeg_destroy(och_jpeg *e)
{
    if (!g_live.remove(e))
        return;
    ochip_jpeg_destroy(e->dev);
    delete e;
}

} // extern "C"
