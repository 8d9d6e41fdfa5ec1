// liboc_host.so: the layered full-resolution orthomosaic (generateLayeredGeoTIFF / processLayeredTile,
// src/ortho/ortho.cpp:1206-1663): the camera table, the CPU route and the C ABI of include/oc_host.h.
//
// The CPU route is the yardstick of the device route (ortho_layers.hip): the reference's loops over a band, the 5 nearest
// cameras by brute force, one OpenMP thread per row, then the correspondences of the finished band tile by tile, in the
// canonical order.  The per-pixel rules are ortho_layers.hpp's, shared with the device.
#include "../../../include/oc_host.h"

#include "../ortho_geom.hpp"
#include "../ortho_layers.hpp"
#include "capi_graph.hpp"
#include "ortho.hpp"
#include "relax_util.hpp"

#include <cstring>
#include <string>
#include <vector>

using namespace opencalibration_amd;

namespace
{

thread_local std::string layers_error;

// the involved nodes' records (ochip_ortho_layers' cams layout), in node order
struct LayerCameras
{
    std::vector<double> cams;
    std::vector<uint64_t> ids;
    std::vector<uint32_t> models;
    std::vector<int64_t> hw; // pixels_rows, pixels_cols
};

LayerCameras layerCameras(const ortho::Context &context, const MeasurementGraph &graph)
{
    LayerCameras out;
    for (size_t i : context.involved)
    {
        const MeasurementGraph::Node &node = graph.nodes()[i];
        const image &p = node.payload;
        // orientation.inverse(): the conjugate over the squared norm; toRotationMatrix() of it
        const double *q = p.orientation;
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        const double qi[4] = {-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2};
        double R[3][3];
        relax_detail::to_matrix(qi, R);
        const CameraModel &m = *p.model;
        double c[ochip_ol::CAM_DOUBLES] = {p.position[0], p.position[1], p.position[2]};
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++)
                c[3 + 3 * r + k] = R[r][k];
        const double model[8] = {m.focal_length_pixels, m.principle_point[0], m.principle_point[1], m.radial_distortion[0],
                                 m.radial_distortion[1], m.radial_distortion[2], m.tangential_distortion[0],
                                 m.tangential_distortion[1]};
        std::copy(model, model + 8, c + 12);
        c[20] = (double)m.pixels_cols;
        c[21] = (double)m.pixels_rows;
        // orientation.inverse() * (0, 0, 1), Eigen's quaternion-vector product: uv = 2 (q.vec x v); v + w uv + q.vec x uv
        const double v[3] = {0, 0, 1};
        double uv[3] = {qi[1] * v[2] - qi[2] * v[1], qi[2] * v[0] - qi[0] * v[2], qi[0] * v[1] - qi[1] * v[0]};
        for (double &u : uv)
            u += u;
        const double cr[3] = {qi[1] * uv[2] - qi[2] * uv[1], qi[2] * uv[0] - qi[0] * uv[2], qi[0] * uv[1] - qi[1] * uv[0]};
        for (int k = 0; k < 3; k++)
            c[22 + k] = v[k] + qi[3] * uv[k] + cr[k];
        out.cams.insert(out.cams.end(), c, c + ochip_ol::CAM_DOUBLES);
        out.ids.push_back(node.id);
        out.models.push_back((uint32_t)m.id);
        out.hw.push_back((int64_t)m.pixels_rows);
        out.hw.push_back((int64_t)m.pixels_cols);
    }
    return out;
}

// The CPU route over one band: heights z [rows][width] (float), outputs as ochip_ortho_layers'.
void layersCPU(const ortho::Plan &plan, const LayerCameras &cams, const uint8_t *const *images, const float *z, int64_t row0,
               int64_t rows, const int32_t *config4, uint8_t *bgra, uint64_t *ids, float *weight, uint32_t *knn_out,
               std::vector<ochip_ol::corr_record> *corr)
{
    ochip_ol::lab_tables tables;
    ochip_ol::lab_tables_build(&tables);
    const int L = config4[0];
    const int64_t W = plan.width;
    const size_t px = (size_t)rows * (size_t)W;
    std::vector<uint8_t> nvalid(px);
    std::vector<uint32_t> cam((size_t)L * px);
    std::vector<float> fields((size_t)L * px * 4);
    const ochip_ol::band_planes B{L, (int32_t)W, rows, nvalid.data(), cam.data(), bgra, ids, weight, fields.data()};
    const ochip_ol::cameras_view C{cams.cams.data(), images, (uint32_t)cams.ids.size()};
    const uint32_t n_cams = (uint32_t)cams.ids.size();
#pragma omp parallel for schedule(dynamic)
    for (int64_t r = 0; r < rows; r++)
        for (int64_t col = 0; col < W; col++)
        {
            const int64_t row = row0 + r;
            const double x = (int)col * plan.gsd + plan.bounds.min_x;
            const double y = plan.bounds.max_y - row * plan.gsd;
            double bd[ochip_og::KNN];
            uint32_t bi[ochip_og::KNN];
            ochip_og::knn_brute(cams.cams.data(), ochip_ol::CAM_DOUBLES, n_cams, x, y, ochip_ol::NONE, bd, bi);
            const size_t i = (size_t)r * W + col;
            if (knn_out)
                std::copy(bi, bi + ochip_og::KNN, knn_out + i * ochip_og::KNN);
            ochip_ol::pixel_layers(tables, C, cams.ids.data(), bi, x, y, z[i], plan.gsd, B, i);
        }
    // the finished band: output tiles row-major, local raster order
    const ochip_ol::corr_config K{config4[1], config4[2], config4[3], row0};
    const int T = K.tile_size;
    for (int64_t tr0 = 0; tr0 < rows; tr0 += T)
        for (int64_t tc0 = 0; tc0 < W; tc0 += T)
            for (int64_t r = tr0; r < std::min<int64_t>(tr0 + T, rows); r++)
                for (int64_t c = tc0; c < std::min<int64_t>(tc0 + T, W); c++)
                {
                    const int n = ochip_ol::corr_count(B, K, r, (int32_t)c);
                    if (n == 0)
                        continue;
                    const size_t at = corr->size();
                    corr->resize(at + n);
                    ochip_ol::corr_write(tables, B, K, cams.models.data(), r, (int32_t)c, corr->data() + at);
                }
}

bool read_plan8(const double *plan8, ortho::Plan *p)
{
    if (!(plan8[0] >= 0 && plan8[0] <= 2147483647.0 && plan8[1] >= 0 && plan8[1] <= 2147483647.0))
        return false;
    p->width = (int)plan8[0];
    p->height = (int)plan8[1];
    p->gsd = plan8[2];
    p->bounds = ortho::Bounds{plan8[3], plan8[4], plan8[5], plan8[6], 0};
    p->mean_camera_z = plan8[7];
    return true;
}

// och_ortho_layers_render (subset == nullptr) and och_ortho_layers_render_subset: `who` names the entry point in errors
int renderLayers(const char *who, const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces,
                 size_t n, const double *plan8, const int32_t *config4, int64_t row0, int64_t rows, const uint32_t *subset,
                 size_t n_subset, const uint64_t *images, const int64_t *image_hw, const float *dsm_in, int out_on_device,
                 uint8_t *bgra, uint64_t *ids, float *weight, ochip_color_corr *corr_out, uint64_t corr_capacity,
                 uint64_t *n_corr, uint32_t *knn_out)
{
    const std::string name = who;
    ortho::Plan plan;
    if (!plan8 || !config4 || !n_corr || !read_plan8(plan8, &plan))
    {
        layers_error = name + ": bad argument";
        return -1;
    }
    const int L = config4[0], T = config4[1];
    if (L < 1 || L > ochip_ol::MAX_LAYERS || T < 1 || config4[2] < 0)
    {
        layers_error = name + ": num_layers 1..8, tile_size >= 1 and kernel radius >= 0";
        return -1;
    }
    if (row0 < 0 || rows < 0 || row0 % T != 0 || row0 + rows > plan.height || (rows % T != 0 && row0 + rows != plan.height))
    {
        layers_error = name + ": a band is whole tile rows from a tile row (the raster's last may be partial)";
        return -1;
    }
    *n_corr = 0;
    std::vector<const surface_model *> surf;
    for (size_t i = 0; i < n; i++)
        surf.push_back(&surfaces[i]->s);
    LayerCameras cams = layerCameras(ortho::prepareContext(surf, g->graph, false), g->graph);
    if (subset)
    {
        // the subset keeps the cameras' order, so the kNN's tie order among its members is the full table's
        LayerCameras part;
        for (size_t j = 0; j < n_subset; j++)
        {
            const size_t i = subset[j];
            if (i >= cams.ids.size() || (j && subset[j] <= subset[j - 1]))
            {
                layers_error = name + ": subset entry " + std::to_string(j) + " is out of range (" + std::to_string(cams.ids.size()) +
                               " involved cameras) or not above the entry before it";
                return -1;
            }
            part.cams.insert(part.cams.end(), cams.cams.begin() + i * ochip_ol::CAM_DOUBLES,
                             cams.cams.begin() + (i + 1) * ochip_ol::CAM_DOUBLES);
            part.ids.push_back(cams.ids[i]);
            part.models.push_back(cams.models[i]);
            part.hw.insert(part.hw.end(), {cams.hw[2 * i], cams.hw[2 * i + 1]});
        }
        cams = std::move(part);
    }
    const size_t nc = cams.ids.size();
    // the kNN lists name rows of the table rendered from: back to och_ortho_layers_cameras' order
    const auto map_knn = [&]() {
        if (subset && knn_out)
            for (size_t i = 0; i < (size_t)rows * (size_t)plan.width * ochip_og::KNN; i++)
                if (knn_out[i] != ochip_ol::NONE)
                    knn_out[i] = subset[knn_out[i]];
    };
    for (size_t i = 0; i < nc; i++)
        if (!images || !images[i] || !image_hw || image_hw[2 * i] != cams.hw[2 * i] || image_hw[2 * i + 1] != cams.hw[2 * i + 1])
        {
            layers_error = name + ": involved camera " + std::to_string(i) + " (node " + std::to_string(cams.ids[i]) +
                           ") has no image or one whose size differs from its model's pixels_rows x pixels_cols";
            return -1;
        }
    const size_t px = (size_t)rows * (size_t)plan.width;
    if (px && (!bgra || !ids))
    {
        layers_error = name + ": bgra and ids are required";
        return -1;
    }
    if (dev)
    {
        if (!ctx)
        {
            layers_error = name + ": the device route needs the mesh's context";
            return -1;
        }
        const double raster4[4] = {plan.bounds.min_x, plan.bounds.max_y, plan.gsd, plan.mean_camera_z};
        const int rc = ochip_ortho_layers(dev, raster4, plan.width, row0, rows, config4, (uint32_t)nc, cams.cams.data(),
                                          cams.ids.data(), cams.models.data(), images, out_on_device, bgra, ids, weight, corr_out,
                                          corr_capacity, n_corr, knn_out);
        if (rc != OCHIP_OK)
        {
            layers_error = std::string("ochip_ortho_layers: ") + ochip_last_error(ctx);
            return -1;
        }
        map_knn();
        return 0;
    }
    if (out_on_device)
    {
        layers_error = name + ": the CPU route writes host memory only";
        return -1;
    }
    std::vector<float> z(px);
    if (dsm_in)
        std::copy(dsm_in, dsm_in + px, z.begin());
    else
    {
        std::vector<double> z64(px);
        ortho::heightsCPU(surf, plan, row0, rows, z64.data(), nullptr, nullptr);
        for (size_t i = 0; i < px; i++)
            z[i] = (float)z64[i];
    }
    std::vector<const uint8_t *> img(nc);
    for (size_t i = 0; i < nc; i++)
        img[i] = reinterpret_cast<const uint8_t *>(images[i]);
    std::vector<ochip_ol::corr_record> corr;
    layersCPU(plan, cams, img.data(), z.data(), row0, rows, config4, bgra, ids, weight, knn_out, &corr);
    *n_corr = corr.size();
    if (corr_out)
        std::memcpy(corr_out, corr.data(), std::min<size_t>(corr.size(), corr_capacity) * sizeof(ochip_color_corr));
    map_knn();
    return 0;
}

} // namespace

extern "C"
{

size_t och_ortho_layers_cameras(const och_graph *g, const och_surface *const *surfaces, size_t n, double *cams,
                                uint64_t *node_ids, uint32_t *model_ids, int64_t *image_hw)
{
    std::vector<const surface_model *> surf;
    for (size_t i = 0; i < n; i++)
        surf.push_back(&surfaces[i]->s);
    const LayerCameras c = layerCameras(ortho::prepareContext(surf, g->graph, false), g->graph);
    if (cams)
        std::copy(c.cams.begin(), c.cams.end(), cams);
    if (node_ids)
        std::copy(c.ids.begin(), c.ids.end(), node_ids);
    if (model_ids)
        std::copy(c.models.begin(), c.models.end(), model_ids);
    if (image_hw)
        std::copy(c.hw.begin(), c.hw.end(), image_hw);
    return c.ids.size();
}

int och_ortho_layers_render(const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces,
                            size_t n, const double *plan8, const int32_t *config4, int64_t row0, int64_t rows,
                            const uint64_t *images, const int64_t *image_hw, const float *dsm_in, int out_on_device,
                            uint8_t *bgra, uint64_t *ids, float *weight, ochip_color_corr *corr_out, uint64_t corr_capacity,
                            uint64_t *n_corr, uint32_t *knn_out)
{
    return renderLayers("och_ortho_layers_render", g, ctx, dev, surfaces, n, plan8, config4, row0, rows, nullptr, 0, images,
                        image_hw, dsm_in, out_on_device, bgra, ids, weight, corr_out, corr_capacity, n_corr, knn_out);
}

int och_ortho_layers_render_subset(const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces,
                                   size_t n, const double *plan8, const int32_t *config4, int64_t row0, int64_t rows,
                                   const uint32_t *subset, size_t n_subset, const uint64_t *images, const int64_t *image_hw,
                                   const float *dsm_in, int out_on_device, uint8_t *bgra, uint64_t *ids, float *weight,
                                   ochip_color_corr *corr_out, uint64_t corr_capacity, uint64_t *n_corr, uint32_t *knn_out)
{
    static const uint32_t none = 0;
    return renderLayers("och_ortho_layers_render_subset", g, ctx, dev, surfaces, n, plan8, config4, row0, rows,
                        subset ? subset : &none, subset ? n_subset : 0, images, image_hw, dsm_in, out_on_device, bgra, ids, weight,
                        corr_out, corr_capacity, n_corr, knn_out);
}

int och_ortho_band_cameras(ochip_ctx *ctx, const double *raster4, int32_t cols, int64_t rows, int64_t band_rows, size_t n_cams,
                           const double *cams, uint8_t *used)
{
    if (!raster4 || cols < 0 || rows < 0 || band_rows < 1 || (n_cams && !cams) || n_cams >= ochip_ol::NONE)
    {
        layers_error = "och_ortho_band_cameras: bad argument";
        return -1;
    }
    const size_t n_bands = (size_t)((rows + band_rows - 1) / band_rows);
    if (n_bands * n_cams == 0)
        return 0;
    if (!used)
    {
        layers_error = "och_ortho_band_cameras: bad argument";
        return -1;
    }
    if (ctx)
    {
        if (ochip_ortho_band_cameras(ctx, raster4, cols, rows, band_rows, (uint32_t)n_cams, cams, used) != OCHIP_OK)
        {
            layers_error = std::string("ochip_ortho_band_cameras: ") + ochip_last_error(ctx);
            return -1;
        }
        return 0;
    }
    // the CPU route: layersCPU's pixel centres, distances and kNN order, brute force; a row's flags are merged per row
    std::fill(used, used + n_bands * n_cams, (uint8_t)0);
    const double min_x = raster4[0], max_y = raster4[1], gsd = raster4[2];
#pragma omp parallel for schedule(dynamic)
    for (int64_t row = 0; row < rows; row++)
    {
        std::vector<uint8_t> mine(n_cams, 0);
        for (int64_t col = 0; col < cols; col++)
        {
            const double x = (int)col * gsd + min_x;
            const double y = max_y - row * gsd;
            double bd[ochip_og::KNN];
            uint32_t bi[ochip_og::KNN];
            ochip_og::knn_brute(cams, ochip_ol::CAM_DOUBLES, n_cams, x, y, ochip_ol::NONE, bd, bi);
            for (int k = 0; k < ochip_og::KNN; k++)
                if (bi[k] != ochip_ol::NONE)
                    mine[bi[k]] = 1;
        }
        uint8_t *band = used + (size_t)(row / band_rows) * n_cams;
        for (size_t i = 0; i < n_cams; i++)
            if (mine[i])
            {
#pragma omp atomic write
                band[i] = 1;
            }
    }
    return 0;
}

const char *och_ortho_layers_last_error(void)
{
    return layers_error.c_str();
}

void och_lab_convert(int mode, const uint8_t *in, size_t n, void *out)
{
    ochip_ol::lab_tables t;
    ochip_ol::lab_tables_build(&t);
    for (size_t i = 0; i < n; i++)
        if (mode == 0)
            ochip_ol::lab8_from_bgr8(t, in + 3 * i, static_cast<uint8_t *>(out) + 3 * i);
        else if (mode == 1)
            ochip_ol::bgr8_from_lab8(t, in + 3 * i, static_cast<uint8_t *>(out) + 3 * i);
        else
            ochip_ol::labf_from_bgr8(t, in + 3 * i, static_cast<float *>(out) + 3 * i);
}

int och_ortho_patch_sample(const double *cam28, const uint8_t *img, double gsd, const double *xyz, uint8_t *bgr_out,
                           double *pixel2, double *J4)
{
    ochip_ol::lab_tables t;
    ochip_ol::lab_tables_build(&t);
    double pixel[2], J[4];
    const double rz = ochip_ol::project_jacobian(cam28, xyz[0], xyz[1], xyz[2], pixel, J);
    if (pixel2)
        pixel2[0] = pixel[0], pixel2[1] = pixel[1];
    if (J4)
        std::memcpy(J4, J, sizeof J);
    const int cols = (int)cam28[20], rows = (int)cam28[21];
    if (rz <= 0 || !(pixel[0] >= 0 && pixel[0] < cols && pixel[1] >= 0 && pixel[1] < rows))
        return 0;
    return ochip_ol::patch_sample(t, img, rows, cols, pixel, J, gsd, bgr_out) ? 1 : 0;
}

void och_ortho_sample_fields(double pixel_x, double pixel_y, int32_t width, int32_t height, float camera_distance,
                             double cos_view, float *out5)
{
    out5[0] = ochip_ol::normalized_radius(pixel_x, pixel_y, width, height);
    ochip_ol::normalized_position(pixel_x, pixel_y, width, height, &out5[1], &out5[2]);
    out5[3] = ochip_ol::blend_weight((float)pixel_x, (float)pixel_y, width, height, camera_distance);
    out5[4] = (float)ochip_ol::acos_restated(cos_view);
}

} // extern "C"
