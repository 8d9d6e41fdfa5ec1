// liboc_host.so: the PNG codec (csrc/png_rules.hpp, png_decode.hpp).  The encoder over both routes -
// the device's kernels, or the shared header's rules in loops, OpenMP over the rows and over the segments of all images of a
// batch and over the images for the assembly - the decoder, which is host code only, and the graph's thumbnails between
// pixels and base64 text.  The CPU route never hands an image to the device by size: it is the yardstick of the device
// route's tests.
#include "../../../include/oc_host.h"

#include "../live_handles.hpp"
#include "capi_graph.hpp"
#include "png_decode.hpp"

#include <memory>
#include <string>
#include <vector>

using namespace opencalibration_amd;

namespace
{
using namespace ochip_png;

thread_local std::string png_error;

int fail(int code, const std::string &text)
{
    png_error = text;
    return code;
}

ochip::live_set<och_png_encoder> g_live; // the encoders that exist

// "" or why the batch is refused; shapes and the sum of the bounds
std::string check_batch(int64_t n, const ochip_png_image *images, int base64, const uint8_t *out, uint64_t out_cap, const uint64_t *offsets,
                        std::vector<shape> &shapes)
{
    if (n < 0 || n > MAX_BATCH)
        return "a batch of " + std::to_string(n) + " images, 0 .. " + std::to_string(MAX_BATCH) + " are taken";
    if ((n && !images) || !out || !offsets)
        return "the images, the output or the offsets are NULL";
    shapes.resize((size_t)n);
    uint64_t need = 0;
    for (int64_t i = 0; i < n; i++)
    {
        const ochip_png_image &m = images[i];
        if (!m.pixels)
            return "image " + std::to_string(i) + " has no pixels";
        if (!make_shape(m.width, m.height, m.channels, m.swap_rb != 0, shapes[(size_t)i]))
            return "image " + std::to_string(i) + ": " + std::to_string(m.width) + " x " + std::to_string(m.height) + " of " +
                   std::to_string(m.channels) + " channels; sides of 1 .. 65535, 1, 3 or 4 channels and a payload below 2^31 bytes are taken";
        const uint64_t bound = file_bound(shapes[(size_t)i].F);
        need += base64 ? base64_bytes(bound) : bound;
    }
    if (out_cap < need)
        return "room for " + std::to_string(out_cap) + " bytes, the bounds of the " + std::to_string(n) + " images add up to " +
               std::to_string(need);
    return "";
}

// The files of a batch in loops: the rows of all images, then the segments of all images, then the images
void encode_batch(const ochip_png_image *images, const std::vector<shape> &shapes, std::vector<std::vector<uint8_t>> &files)
{
    const size_t n = shapes.size();
    std::vector<std::vector<uint8_t>> payload(n);
    std::vector<std::vector<uint16_t>> marks(n);
    std::vector<std::vector<block_out>> blocks(n);
    std::vector<uint64_t> row_base(n + 1, 0), seg_base(n + 1, 0);
    for (size_t i = 0; i < n; i++)
    {
        payload[i].resize((size_t)shapes[i].F), marks[i].resize((size_t)shapes[i].F), blocks[i].resize(shapes[i].segs);
        row_base[i + 1] = row_base[i] + shapes[i].h, seg_base[i + 1] = seg_base[i] + shapes[i].segs;
    }
    auto owner = [](const std::vector<uint64_t> &base, uint64_t u) {
        size_t lo = 0, hi = base.size() - 1; // base[lo] <= u < base[hi]
        while (hi - lo > 1)
        {
            const size_t mid = (lo + hi) / 2;
            (base[mid] <= u ? lo : hi) = mid;
        }
        return lo;
    };
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t u = 0; u < (int64_t)row_base[n]; u++)
    {
        const size_t i = owner(row_base, (uint64_t)u);
        const uint32_t y = (uint32_t)((uint64_t)u - row_base[i]);
        filter_row(static_cast<const uint8_t *>(images[i].pixels), shapes[i], y, payload[i].data() + (size_t)y * shapes[i].stride);
    }
#pragma omp parallel for schedule(dynamic)
    for (int64_t u = 0; u < (int64_t)seg_base[n]; u++)
    {
        const size_t i = owner(seg_base, (uint64_t)u);
        const uint32_t k = (uint32_t)((uint64_t)u - seg_base[i]);
        segment_block(payload[i].data(), shapes[i].F, k, shapes[i].dist_left(), shapes[i].dist_up(), marks[i].data(), blocks[i][k]);
    }
    files.resize(n);
#pragma omp parallel for schedule(dynamic)
    for (int64_t i = 0; i < (int64_t)n; i++)
        assemble_file(payload[(size_t)i].data(), shapes[(size_t)i], marks[(size_t)i].data(), blocks[(size_t)i].data(), files[(size_t)i]);
}

int base64_value(char ch)
{
    return ch >= 'A' && ch <= 'Z' ? ch - 'A' : ch >= 'a' && ch <= 'z' ? ch - 'a' + 26 : ch >= '0' && ch <= '9' ? ch - '0' + 52 : ch == '+' ? 62 : ch == '/' ? 63 : -1;
}

// RFC 4648 with padding; line breaks are skipped (OpenSSL-style writers emit them).  false: not base64
bool base64_decode(const std::string &text, std::vector<uint8_t> &out)
{
    out.clear();
    uint32_t acc = 0;
    int have = 0, pad = 0;
    for (char ch : text)
    {
        if (ch == '\n' || ch == '\r')
            continue;
        if (ch == '=')
        {
            pad++;
            continue;
        }
        const int v = base64_value(ch);
        if (v < 0 || pad)
            return false;
        acc = acc << 6 | (uint32_t)v, have++;
        if (have == 4)
            out.push_back((uint8_t)(acc >> 16)), out.push_back((uint8_t)(acc >> 8)), out.push_back((uint8_t)acc), acc = 0, have = 0;
    }
    if (have == 1 || pad > 2 || (have == 0 && pad) || (have && have + pad != 4))
        return false;
    if (have == 2)
        out.push_back((uint8_t)(acc >> 4));
    else if (have == 3)
        out.push_back((uint8_t)(acc >> 10)), out.push_back((uint8_t)(acc >> 2));
    return true;
}
} // namespace

struct och_png_encoder
{
    ochip_ctx *ctx = nullptr;
    ochip_png_encoder *dev = nullptr; // the device route
};

extern "C"
{

const char *och_png_last_error(void)
{
    return png_error.c_str();
}

uint64_t och_png_bound(int64_t width, int64_t height, int64_t channels, int base64)
{
    shape s;
    if (!make_shape(width, height, channels, false, s))
        return 0;
    return base64 ? base64_bytes(file_bound(s.F)) : file_bound(s.F);
}

int och_png_encoder_create(ochip_ctx *ctx, och_png_encoder **out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_png_encoder_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<och_png_encoder> e(new och_png_encoder);
    e->ctx = ctx;
    if (ctx)
    {
        const int rc = ochip_png_encoder_create(ctx, &e->dev);
        if (rc != OCHIP_OK)
            return fail(rc, ochip_last_error(ctx));
    }
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

int och_png_encoder_encode(och_png_encoder *e, int64_t n, const ochip_png_image *images, int on_device, int base64, uint8_t *out,
                           uint64_t out_cap, uint64_t *offsets)
{
    if (!g_live.has(e))
        return fail(OCHIP_EINVAL, "och_png_encoder_encode: not a live och_png_encoder object");
    if (e->dev)
    {
        const int rc = ochip_png_encoder_encode(e->dev, n, images, on_device, base64, out, out_cap, offsets);
        return rc == OCHIP_OK ? rc : fail(rc, ochip_last_error(e->ctx));
    }
    if (on_device)
        return fail(OCHIP_EINVAL, "och_png_encoder_encode: images on the device need a device context");
    std::vector<shape> shapes;
    const std::string refusal = check_batch(n, images, base64, out, out_cap, offsets, shapes);
    if (!refusal.empty())
        return fail(OCHIP_EINVAL, "och_png_encoder_encode: " + refusal);
    std::vector<std::vector<uint8_t>> files;
    encode_batch(images, shapes, files);
    offsets[0] = 0;
    for (size_t i = 0; i < files.size(); i++)
        offsets[i + 1] = offsets[i] + (base64 ? base64_bytes(files[i].size()) : files[i].size());
#pragma omp parallel for schedule(dynamic)
    for (int64_t i = 0; i < (int64_t)files.size(); i++)
    {
        const std::vector<uint8_t> &f = files[(size_t)i];
        if (base64)
            base64_encode(f.data(), f.size(), reinterpret_cast<char *>(out + offsets[i]));
        else
            std::memcpy(out + offsets[i], f.data(), f.size());
    }
    return OCHIP_OK;
}

void och_png_encoder_destroy(och_png_encoder *e)
{
    if (!g_live.remove(e))
        return;
    ochip_png_encoder_destroy(e->dev);
    delete e;
}

int och_png_filter(const ochip_png_image *image, uint8_t *payload, uint64_t cap)
{
    shape s;
    if (!image || !image->pixels || !payload || !make_shape(image->width, image->height, image->channels, image->swap_rb != 0, s) || cap < s.F)
        return fail(OCHIP_EINVAL, "och_png_filter: a NULL argument, a shape that is not taken or too little room");
    for (uint32_t y = 0; y < s.h; y++)
        filter_row(static_cast<const uint8_t *>(image->pixels), s, y, payload + (size_t)y * s.stride);
    return OCHIP_OK;
}

static void copy_info(const file_info &I, och_png_file_info *out)
{
    out->width = I.width, out->height = I.height, out->bit_depth = I.bit_depth, out->color_type = I.color_type;
    out->interlace = I.interlace, out->channels = I.channels, out->status = I.status;
}

int och_png_info(const uint8_t *data, uint64_t size, och_png_file_info *out)
{
    if (!out)
        return fail(OCHIP_EINVAL, "och_png_info: out is NULL");
    file_info I;
    read_info(data, data ? size : 0, I);
    copy_info(I, out);
    return OCHIP_OK;
}

int och_png_decode(const uint8_t *data, uint64_t size, och_png_file_info *info, uint8_t **pixels)
{
    if (!info || !pixels)
        return fail(OCHIP_EINVAL, "och_png_decode: info or pixels is NULL");
    *pixels = nullptr;
    file_info I;
    std::vector<uint8_t> px;
    decode_file(data, data ? size : 0, I, px);
    copy_info(I, info);
    if (I.status != PNG_OK)
        return OCHIP_OK;
    *pixels = static_cast<uint8_t *>(std::malloc(px.size()));
    if (!*pixels)
        return fail(OCHIP_ENOMEM, "och_png_decode: no memory for the picture");
    std::memcpy(*pixels, px.data(), px.size());
    return OCHIP_OK;
}

void och_png_free(uint8_t *pixels)
{
    std::free(pixels);
}

int och_graph_get_thumbnail(och_graph *g, size_t node_index, size_t *rows, size_t *cols, uint8_t *rgb)
{
    if (!g)
        return -1;
    if (node_index >= g->graph.size_nodes() || !rows || !cols)
    {
        g->error = "och_graph_get_thumbnail: bad node index, or no place for the size";
        return -1;
    }
    const image &p = g->graph.nodes()[node_index].payload;
    *rows = p.thumbnail_rows, *cols = p.thumbnail_cols;
    if (rgb && !p.thumbnail_pixels.empty())
        std::memcpy(rgb, p.thumbnail_pixels.data(), p.thumbnail_pixels.size());
    return 0;
}

int och_graph_encode_thumbnails(och_graph *g, ochip_ctx *ctx)
{
    if (!g)
        return -1;
    std::vector<size_t> nodes;
    std::vector<ochip_png_image> images;
    uint64_t cap = 0;
    for (size_t k = 0; k < g->graph.size_nodes(); k++)
    {
        const image &p = g->graph.nodes()[k].payload;
        if (p.thumbnail_rows == 0 || p.thumbnail_cols == 0 || p.thumbnail_pixels.size() != p.thumbnail_rows * p.thumbnail_cols * 3)
            continue;
        const uint64_t bound = och_png_bound((int64_t)p.thumbnail_cols, (int64_t)p.thumbnail_rows, 3, 1);
        if (bound == 0)
        {
            g->error = "och_graph_encode_thumbnails: the thumbnail of node index " + std::to_string(k) + " is too large for a PNG";
            return -1;
        }
        nodes.push_back(k), cap += bound;
        images.push_back(ochip_png_image{p.thumbnail_pixels.data(), (int32_t)p.thumbnail_cols, (int32_t)p.thumbnail_rows, 3, 0});
    }
    if (nodes.empty())
        return 0;
    if (nodes.size() > (size_t)MAX_BATCH)
    {
        g->error = "och_graph_encode_thumbnails: more than 65535 thumbnails";
        return -1;
    }
    och_png_encoder *e = nullptr;
    if (och_png_encoder_create(ctx, &e) != OCHIP_OK)
    {
        g->error = "och_graph_encode_thumbnails: " + png_error;
        return -1;
    }
    std::vector<uint8_t> text((size_t)cap);
    std::vector<uint64_t> offsets(nodes.size() + 1);
    const int rc = och_png_encoder_encode(e, (int64_t)nodes.size(), images.data(), 0, 1, text.data(), cap, offsets.data());
    och_png_encoder_destroy(e);
    if (rc != OCHIP_OK)
    {
        g->error = "och_graph_encode_thumbnails: " + png_error;
        return -1;
    }
    for (size_t i = 0; i < nodes.size(); i++)
        g->graph.nodes()[nodes[i]].payload.thumbnail_b64.assign(reinterpret_cast<const char *>(text.data()) + offsets[i],
                                                                (size_t)(offsets[i + 1] - offsets[i]));
    return (int)nodes.size();
}

int och_graph_decode_thumbnails(och_graph *g, int32_t *statuses)
{
    if (!g)
        return -1;
    const size_t n = g->graph.size_nodes();
    std::vector<int32_t> st(n, -1);
    std::vector<file_info> infos(n);
    std::vector<std::vector<uint8_t>> rgb(n);
#pragma omp parallel for schedule(dynamic)
    for (int64_t k = 0; k < (int64_t)n; k++)
    {
        const image &p = g->graph.nodes()[(size_t)k].payload;
        if (p.thumbnail_b64.empty())
            continue;
        std::vector<uint8_t> file, px;
        if (!base64_decode(p.thumbnail_b64, file))
        {
            st[(size_t)k] = PNG_CORRUPT;
            continue;
        }
        st[(size_t)k] = decode_file(file.data(), file.size(), infos[(size_t)k], px);
        if (st[(size_t)k] == PNG_OK && (infos[(size_t)k].width > 65535 || infos[(size_t)k].height > 65535))
            st[(size_t)k] = PNG_UNSUPPORTED; // beyond what a node's thumbnail may be (och_graph_set_thumbnail)
        if (st[(size_t)k] == PNG_OK)
            to_three_channels(px, infos[(size_t)k], rgb[(size_t)k]);
    }
    int taken = 0;
    for (size_t k = 0; k < n; k++)
    {
        if (statuses)
            statuses[k] = st[k];
        if (st[k] != PNG_OK)
            continue; // a refused node is left as it was
        image &p = g->graph.nodes()[k].payload;
        p.thumbnail_rows = infos[k].height, p.thumbnail_cols = infos[k].width;
        p.thumbnail_pixels.swap(rgb[k]);
        taken++;
    }
    return taken;
}

} // extern "C"
