// liboc_host.so: the load stage's image thumbnails (csrc/thumbnail.hpp; src/extract/extract_image.cpp:42-52).  The CPU
// route - the rules of the shared header in straight loops, OpenMP over rows - and the C ABI over both routes.
#include "../../../include/oc_host.h"

#include "../area_table.hpp"
#include "../thumbnail.hpp"
#include "capi_graph.hpp"

#include <string>
#include <vector>

using namespace opencalibration_amd;

namespace
{

thread_local std::string thumbnail_error;

// one image: bgr [height][width][3] -> rgb [P.rows][P.cols][3]
void thumbnail_cpu(const ochip_ol::lab_tables &T, const ochip_th::plan &P, const area_tab &tx, const area_tab &ty,
                   const uint8_t *bgr, int width, int height, uint8_t *rgb)
{
    const size_t row_values = (size_t)P.cols * 3;
    std::vector<uint8_t> lab8((size_t)P.rows * row_values);
    if (P.n > 0)
    {
        // integer path: per source row the integer sums of each cell's in-range columns, then the cells
        std::vector<uint32_t> sums((size_t)height * row_values);
#pragma omp parallel for schedule(static)
        for (int y = 0; y < height; y++)
        {
            std::vector<uint32_t> lab((size_t)width);
            for (int x = 0; x < width; x++)
            {
                const uint8_t *p = bgr + ((size_t)y * width + x) * 3;
                lab[x] = ochip_th::lab_word(T, (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
            }
            for (int dx = 0; dx < P.cols; dx++)
            {
                int x0, nx;
                ochip_th::cell_range(dx, P.n, width, &x0, &nx);
                for (int c = 0; c < 3; c++)
                {
                    uint32_t s = 0;
                    for (int k = 0; k < nx; k++)
                        s += lab[x0 + k] >> (8 * c) & 255u;
                    sums[(size_t)y * row_values + (size_t)dx * 3 + c] = s;
                }
            }
        }
#pragma omp parallel for schedule(static)
        for (int dy = 0; dy < P.rows; dy++)
        {
            int y0, ny;
            ochip_th::cell_range(dy, P.n, height, &y0, &ny);
            for (int dx = 0; dx < P.cols; dx++)
            {
                int x0, nx;
                ochip_th::cell_range(dx, P.n, width, &x0, &nx);
                for (int c = 0; c < 3; c++)
                {
                    uint32_t s = 0;
                    for (int k = 0; k < ny; k++)
                        s += sums[(size_t)(y0 + k) * row_values + (size_t)dx * 3 + c];
                    lab8[(size_t)dy * row_values + (size_t)dx * 3 + c] = ochip_th::cell_value(s, nx, ny, P.n);
                }
            }
        }
    }
    else
    {
        // general path: per source row and channel the horizontal taps in table order, then the vertical taps
        std::vector<float> sums((size_t)height * row_values);
#pragma omp parallel for schedule(static)
        for (int y = 0; y < height; y++)
        {
            std::vector<uint32_t> lab((size_t)width);
            for (int x = 0; x < width; x++)
            {
                const uint8_t *p = bgr + ((size_t)y * width + x) * 3;
                lab[x] = ochip_th::lab_word(T, (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
            }
            for (int dx = 0; dx < P.cols; dx++)
                for (int c = 0; c < 3; c++)
                {
                    float acc = 0.0f;
                    for (int k = tx.off[dx]; k < tx.off[dx + 1]; k++)
                        acc = ochip_th::tap(acc, (float)(lab[tx.si[k]] >> (8 * c) & 255u), tx.alpha[k]);
                    sums[(size_t)y * row_values + (size_t)dx * 3 + c] = acc;
                }
        }
#pragma omp parallel for schedule(static)
        for (int dy = 0; dy < P.rows; dy++)
            for (size_t v = 0; v < row_values; v++)
            {
                float acc = 0.0f;
                for (int e = ty.off[dy]; e < ty.off[dy + 1]; e++)
                    acc = ochip_th::tap(acc, sums[(size_t)ty.si[e] * row_values + v], ty.alpha[e]);
                lab8[(size_t)dy * row_values + v] = ochip_th::round8(acc);
            }
    }
    for (size_t i = 0; i < (size_t)P.rows * P.cols; i++)
        ochip_th::rgb_from_lab8(T, &lab8[3 * i], rgb + 3 * i);
}

int thumbnails(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height, int images_on_device,
               uint8_t *rgb_out, std::string *error)
{
    ochip_th::plan P;
    const int bad = ochip_th::make_plan(width, height, &P);
    if (bad)
    {
        *error = std::string("thumbnails: ") + ochip_th::size_error(bad);
        return -1;
    }
    if (n_images && (!images_bgr || !rgb_out))
    {
        *error = "thumbnails: a NULL image or output pointer";
        return -1;
    }
    if (ctx)
    {
        if (ochip_image_thumbnails(ctx, images_bgr, n_images, width, height, images_on_device, rgb_out) != OCHIP_OK)
        {
            *error = std::string("ochip_image_thumbnails: ") + ochip_last_error(ctx);
            return -1;
        }
        return 0;
    }
    if (images_on_device)
    {
        *error = "thumbnails: images on the device need a device context";
        return -1;
    }
    ochip_ol::lab_tables T;
    ochip_ol::lab_tables_build(&T);
    area_tab tx, ty;
    if (P.n == 0)
    {
        tx = area_table(width, P.cols, P.inv_scale);
        ty = area_table(height, P.rows, P.inv_scale);
    }
    const size_t src = (size_t)width * height * 3, dst = (size_t)P.rows * P.cols * 3;
    for (uint32_t i = 0; i < n_images; i++)
        thumbnail_cpu(T, P, tx, ty, images_bgr + i * src, width, height, rgb_out + i * dst);
    return 0;
}

} // namespace

extern "C"
{

const char *och_thumbnail_last_error(void)
{
    return thumbnail_error.c_str();
}

int och_thumbnail_size(int width, int height, int32_t *rows, int32_t *cols)
{
    ochip_th::plan P;
    const int bad = ochip_th::make_plan(width, height, &P);
    if (bad || !rows || !cols)
    {
        thumbnail_error = std::string("och_thumbnail_size: ") + (bad ? ochip_th::size_error(bad) : "a NULL output pointer");
        return -1;
    }
    *rows = P.rows, *cols = P.cols;
    return 0;
}

int och_image_thumbnails(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                         int images_on_device, uint8_t *rgb_out)
{
    return thumbnails(ctx, images_bgr, n_images, width, height, images_on_device, rgb_out, &thumbnail_error);
}

int och_graph_make_thumbnails(och_graph *g, ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                              int images_on_device, const uint64_t *node_ids)
{
    if (!g)
        return -1;
    if (n_images && !node_ids)
    {
        g->error = "och_graph_make_thumbnails: node_ids is NULL";
        return -1;
    }
    for (uint32_t i = 0; i < n_images; i++)
        if (!g->graph.getNode(node_ids[i]))
        {
            g->error = "och_graph_make_thumbnails: no node " + std::to_string(node_ids[i]);
            return -1;
        }
    ochip_th::plan P;
    const int bad = ochip_th::make_plan(width, height, &P);
    if (bad)
    {
        g->error = std::string("och_graph_make_thumbnails: ") + ochip_th::size_error(bad);
        return -1;
    }
    const size_t dst = (size_t)P.rows * P.cols * 3;
    std::vector<uint8_t> rgb((size_t)n_images * dst);
    if (thumbnails(ctx, images_bgr, n_images, width, height, images_on_device, rgb.data(), &g->error) != 0)
        return -1;
    for (uint32_t i = 0; i < n_images; i++)
    {
        image &p = g->graph.nodes()[g->graph.nodeIndex(node_ids[i])].payload;
        p.thumbnail_rows = (size_t)P.rows;
        p.thumbnail_cols = (size_t)P.cols;
        p.thumbnail_pixels.assign(rgb.begin() + i * dst, rgb.begin() + (i + 1) * dst);
    }
    return 0;
}

} // extern "C"
