// liboc_host.so: the blended full-resolution orthomosaic (blendLayeredGeoTIFF, src/ortho/ortho.cpp:1665-1990, and
// laplacianBlend, src/ortho/blending.cpp): the id table, the CPU route and the C ABI of include/oc_host.h.
//
// The CPU route is the yardstick of the device route (ortho_blend.hip): the reference's tile loop, one OpenMP thread per
// tile, with the sequential two-pass chamfer.  The per-pixel and per-level rules are ortho_blend.hpp's, shared with the
// device.
#include "../../../include/oc_host.h"

#include "../ortho_blend.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace
{

thread_local std::string blend_error;

// laplacianBlend's steps over every tile of `tiles`, each tile by one thread
void levelsCPU(const ochip_ob::arena &A, const std::vector<ochip_ob::tile_info> &tiles, size_t k)
{
    const ochip_ob::tile_info &t = tiles[k];
    auto each = [&](int lv, auto f) {
        for (int y = 0; y < t.lh[lv]; y++)
            for (int x = 0; x < t.lw[lv]; x++)
                f(x, y);
    };
    for (int l = 0; l < A.L; l++)
    {
        for (int lv = 1; lv < t.lf; lv++)
            each(lv, [&](int x, int y) { ochip_ob::fill_down_px(A, t, l, lv, x, y); });
        for (int lv = t.lf - 1; lv >= 0; lv--)
            each(lv, [&](int x, int y) { ochip_ob::fill_up_px(A, t, l, lv, x, y); });
        for (int lv = 1; lv < t.p; lv++)
            each(lv, [&](int x, int y) { ochip_ob::gauss_down_px(A, t, l, lv, x, y); });
    }
    for (int lv = 0; lv < t.p; lv++)
        each(lv, [&](int x, int y) { ochip_ob::blend_px(A, t, lv, x, y); });
    for (int lv = t.p - 2; lv >= 0; lv--)
        each(lv, [&](int x, int y) { ochip_ob::recon_px(A, t, lv, x, y); });
}

struct arena_store
{
    std::vector<float> wr, wc, fl, g, bl;
    ochip_ob::arena A;
    arena_store(int L, int64_t n) : wr((size_t)L * n), wc((size_t)L * n * 3), fl((size_t)L * n * 3), g((size_t)L * n * 3),
                                    bl((size_t)n * 3)
    {
        A = ochip_ob::arena{L, n, wr.data(), wc.data(), fl.data(), g.data(), bl.data()};
    }
};

// the CPU route over one band (ochip_ortho_blend's arguments, host memory)
void blendCPU(const double *raster3, int32_t cols, int64_t row0, int64_t rows, const int32_t *config4, const double *cams,
              const std::vector<ochip_ob::id_entry> &ids, const double *vig0, const uint8_t *bgra, const uint64_t *id,
              const float *dsm, uint8_t *rgba, float *weight_out, float *dist_out, float *lab_out)
{
    const int L = config4[0], TS = config4[1];
    const size_t px = (size_t)rows * (size_t)cols;
    ochip_ol::lab_tables T;
    ochip_ol::lab_tables_build(&T);
    std::vector<ochip_ob::tile_info> tiles;
    const int64_t n = ochip_ob::tiles_build(TS, rows, cols, config4[2], &tiles);
    arena_store S(L, n);
    std::vector<uint8_t> valid((size_t)L * px);
    std::vector<float> weight((size_t)L * px), lab((size_t)L * px * 3);
    std::vector<int32_t> dist(px);
    const ochip_ob::band_view B{L,           cols,  rows,         row0,       raster3[0], raster3[1], raster3[2],
                                bgra,        id,    dsm,          valid.data(), weight.data(), lab.data(), dist.data()};
    const ochip_ob::color_model0 M0{vig0 ? 1 : 0, {vig0 ? vig0[0] : 0, vig0 ? vig0[1] : 0, vig0 ? vig0[2] : 0}};
    const float steepness = (float)std::log(99.0) / (float)config4[3];
#pragma omp parallel for schedule(dynamic)
    for (size_t k = 0; k < tiles.size(); k++)
    {
        const ochip_ob::tile_info &t = tiles[k];
        for (int32_t r = 0; r < t.th; r++)
            for (int32_t c = 0; c < t.tw; c++)
                ochip_ob::prep_pixel(T, B, cams, ids.data(), (uint32_t)ids.size(), M0, t.r0 + r, t.c0 + c);
        ochip_ob::chamfer_tile(B, t);
        for (int32_t r = 0; r < t.th; r++)
            for (int32_t c = 0; c < t.tw; c++)
                ochip_ob::weights_px(B, S.A, t, steepness, t.r0 + r, t.c0 + c);
        levelsCPU(S.A, tiles, k);
        for (int32_t r = 0; r < t.th; r++)
            for (int32_t c = 0; c < t.tw; c++)
                ochip_ob::final_px(T, B, S.A, t, t.r0 + r, t.c0 + c, rgba);
    }
    if (weight_out)
        std::copy(weight.begin(), weight.end(), weight_out);
    if (lab_out)
        std::copy(lab.begin(), lab.end(), lab_out);
    if (dist_out)
        for (size_t i = 0; i < px; i++)
            dist_out[i] = ochip_ob::dist_float(dist[i]);
}

bool read_plan8(const double *plan8, int32_t *width, int32_t *height)
{
    if (!(plan8[0] >= 0 && plan8[0] <= 2147483647.0 && plan8[1] >= 0 && plan8[1] <= 2147483647.0))
        return false;
    *width = (int32_t)plan8[0];
    *height = (int32_t)plan8[1];
    return true;
}

} // namespace

extern "C"
{

int och_ortho_blend_render(const och_graph *g, ochip_ctx *ctx, const och_surface *const *surfaces, size_t n,
                           const double *plan8, const int32_t *config4, int64_t row0, int64_t rows, size_t n_color,
                           const uint64_t *color_ids, const double *color6, size_t n_models, const uint32_t *model_ids,
                           const double *vig3, int on_device, const uint8_t *bgra, const uint64_t *ids, const float *dsm,
                           uint8_t *rgba, float *weight_out, float *dist_out, float *lab_out)
{
    int32_t width = 0, height = 0;
    if (!g || !plan8 || !config4 || !read_plan8(plan8, &width, &height) || (n_color && (!color_ids || !color6)) ||
        (n_models && (!model_ids || !vig3)))
    {
        blend_error = "och_ortho_blend_render: bad argument";
        return -1;
    }
    const int L = config4[0], T = config4[1];
    if (L < 1 || L > ochip_ob::MAX_LAYERS || T < 1 || T > ochip_ob::MAX_TILE || config4[3] < 1)
    {
        blend_error = "och_ortho_blend_render: num_layers 1..8, tile_size 1..4096 and blend_transition_radius >= 1";
        return -1;
    }
    if (row0 < 0 || rows < 0 || row0 % T != 0 || row0 + rows > height || (rows % T != 0 && row0 + rows != height))
    {
        blend_error = "och_ortho_blend_render: a band is whole tile rows from a tile row (the raster's last may be partial)";
        return -1;
    }
    const size_t px = (size_t)rows * (size_t)width;
    if (px && (!bgra || !ids || !dsm || !rgba))
    {
        blend_error = "och_ortho_blend_render: bgra, ids, dsm and rgba are required";
        return -1;
    }
    // the camera table, then the id table: every camera's id and every colour entry's, sorted
    const size_t nc = och_ortho_layers_cameras(g, surfaces, n, nullptr, nullptr, nullptr, nullptr);
    std::vector<double> cams(nc * ochip_ol::CAM_DOUBLES);
    std::vector<uint64_t> node_ids(nc);
    och_ortho_layers_cameras(g, surfaces, n, cams.data(), node_ids.data(), nullptr, nullptr);
    std::vector<ochip_ob::id_entry> table;
    for (size_t i = 0; i < nc; i++)
    {
        ochip_ob::id_entry e{};
        e.id = node_ids[i], e.cam = (uint32_t)i;
        table.push_back(e);
    }
    for (size_t i = 0; i < n_color; i++)
    {
        ochip_ob::id_entry e{};
        e.id = color_ids[i], e.cam = ochip_ob::NONE;
        table.push_back(e);
    }
    std::stable_sort(table.begin(), table.end(), [](const ochip_ob::id_entry &a, const ochip_ob::id_entry &b) { return a.id < b.id; });
    std::vector<ochip_ob::id_entry> uniq;
    for (const auto &e : table)
        if (uniq.empty() || uniq.back().id != e.id)
            uniq.push_back(e);
        else if (e.cam != ochip_ob::NONE)
            uniq.back().cam = e.cam;
    for (size_t i = 0; i < n_color; i++)
    {
        ochip_ob::id_entry &e = uniq[ochip_ob::find_id(uniq.data(), (uint32_t)uniq.size(), color_ids[i])];
        e.has_color = 1;
        std::memcpy(e.offset, color6 + 6 * i, 3 * sizeof(double));
        e.brdf = color6[6 * i + 3];
        e.slope[0] = color6[6 * i + 4], e.slope[1] = color6[6 * i + 5];
    }
    const double *vig0 = nullptr; // readLayeredTileFromGeoTIFF never sets model_id: model 0's entry, or none
    for (size_t i = 0; i < n_models; i++)
        if (model_ids[i] == 0)
            vig0 = vig3 + 3 * i;
    const double raster3[3] = {plan8[3], plan8[6], plan8[2]};
    if (ctx)
    {
        const int rc = ochip_ortho_blend(ctx, raster3, width, row0, rows, config4, (uint32_t)nc, cams.data(),
                                         (uint32_t)uniq.size(), reinterpret_cast<const ochip_blend_id *>(uniq.data()), vig0,
                                         on_device, bgra, ids, dsm, rgba, weight_out, dist_out, lab_out);
        if (rc != OCHIP_OK)
        {
            blend_error = std::string("ochip_ortho_blend: ") + ochip_last_error(ctx);
            return -1;
        }
        return 0;
    }
    if (on_device)
    {
        blend_error = "och_ortho_blend_render: the CPU route reads and writes host memory only";
        return -1;
    }
    if (px)
        blendCPU(raster3, width, row0, rows, config4, cams.data(), uniq, vig0, bgra, ids, dsm, rgba, weight_out, dist_out,
                 lab_out);
    return 0;
}

const char *och_ortho_blend_last_error(void)
{
    return blend_error.c_str();
}

int och_laplacian_blend(int32_t num_layers, int32_t rows, int32_t cols, int32_t pyramid_levels, const float *lab,
                        const float *weight, uint8_t *bgra_out)
{
    if (num_layers < 1 || num_layers > ochip_ob::MAX_LAYERS || rows < 0 || cols < 0 || rows > ochip_ob::MAX_TILE ||
        cols > ochip_ob::MAX_TILE)
        return -1;
    const size_t px = (size_t)rows * (size_t)cols;
    if (px == 0)
        return 0;
    ochip_ol::lab_tables T;
    ochip_ol::lab_tables_build(&T);
    std::vector<ochip_ob::tile_info> tiles;
    const int64_t n = ochip_ob::tiles_build(std::max(rows, cols), rows, cols, pyramid_levels, &tiles);
    arena_store S(num_layers, n);
    float w[ochip_ob::MAX_LAYERS];
    for (size_t k = 0; k < px; k++)
    {
        for (int l = 0; l < num_layers; l++)
            w[l] = weight[(size_t)l * px + k];
        ochip_ob::unity_px(S.A, (int64_t)k, w, lab + 3 * k, 3 * px);
    }
    levelsCPU(S.A, tiles, 0);
    for (size_t k = 0; k < px; k++)
    {
        ochip_ob::blended_bgr8(T, S.A, k, bgra_out + 4 * k);
        bgra_out[4 * k + 3] = 255;
    }
    return 0;
}

void och_blend_chamfer(int32_t rows, int32_t cols, const uint8_t *boundary, int32_t *dist)
{
    ochip_ob::chamfer_seq(
        rows, cols, [&](int32_t r, int32_t c) { return boundary[(size_t)r * cols + c] != 0; },
        [&](int32_t r, int32_t c) -> int32_t & { return dist[(size_t)r * cols + c]; });
}

void och_blend_pyr(int up, int32_t channels, int32_t w, int32_t h, int32_t W, int32_t H, const float *src, float *out)
{
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++)
        {
            float *o = out + ((size_t)y * W + x) * channels;
            if (channels == 1)
                up ? ochip_ob::pyr_up_px<1>(src, w, W, H, x, y, o) : ochip_ob::pyr_down_px<1>(src, w, h, x, y, o);
            else
                up ? ochip_ob::pyr_up_px<3>(src, w, W, H, x, y, o) : ochip_ob::pyr_down_px<3>(src, w, h, x, y, o);
        }
}

void och_blend_math(int mode, size_t n, const float *in, void *out)
{
    ochip_ol::lab_tables T;
    ochip_ol::lab_tables_build(&T);
    for (size_t i = 0; i < n; i++)
        if (mode == 0)
            static_cast<float *>(out)[i] = ochip_ob::exp_restated(in[i]);
        else if (mode == 1)
            static_cast<float *>(out)[i] = ochip_ob::falloff(in[2 * i], in[2 * i + 1]);
        else
            ochip_ob::bgr8_from_labf(T, in + 3 * i, static_cast<uint8_t *>(out) + 3 * i);
}

} // extern "C"
