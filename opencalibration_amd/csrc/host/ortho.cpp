// The orthomosaic preview and the DSM raster on the host: the reference's context (src/ortho/ortho.cpp:228-472) and the
// CPU route of its per-pixel loops (:539-633, :806-853).  See ortho.hpp.
#include "ortho.hpp"

#include "../ortho_geom.hpp"
#include "invert_distortion.hpp"
#include "relax_util.hpp"
#include "triangle_walker.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace opencalibration_amd
{
namespace ortho
{

using relax_detail::TriangleWalker;

namespace
{
constexpr uint32_t MISS = 0xFFFFFFFFu;

void corners(const MeshGraph &mesh, const std::array<size_t, 3> &n, double c9[9])
{
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++)
            c9[3 * i + k] = mesh.nodes[n[i]].location[k];
}
} // namespace

Bounds calculateBoundsAndMeanZ(const std::vector<const surface_model *> &surfaces)
{
    const double inf = std::numeric_limits<double>::infinity();
    double min_x = inf, min_y = inf, max_x = -inf, max_y = -inf;
    std::vector<double> z_values;
    auto take = [&](const double *loc, double &s_min_x, double &s_max_x, double &s_min_y, double &s_max_y) {
        if (std::isfinite(loc[2]))
            z_values.push_back(loc[2]);
        s_min_x = std::min(s_min_x, loc[0]);
        s_max_x = std::max(s_max_x, loc[0]);
        s_min_y = std::min(s_min_y, loc[1]);
        s_max_y = std::max(s_max_y, loc[1]);
    };
    for (const surface_model *surface : surfaces)
    {
        double s_min_x = inf, s_max_x = -inf, s_min_y = inf, s_max_y = -inf;
        for (const MeshNode &n : surface->mesh.nodes)
            take(n.location, s_min_x, s_max_x, s_min_y, s_max_y);
        if (surface->mesh.nodes.empty()) // the clouds only for a surface without a mesh
            for (const point_cloud &points : surface->cloud)
                for (const auto &p : points)
                    take(p.data(), s_min_x, s_max_x, s_min_y, s_max_y);
        min_x = std::min(min_x, s_min_x);
        max_x = std::max(max_x, s_max_x);
        min_y = std::min(min_y, s_min_y);
        max_y = std::max(max_y, s_max_y);
    }
    double mean_surface_z = 0;
    for (double z : z_values)
        mean_surface_z += z;
    if (!z_values.empty())
        mean_surface_z /= z_values.size();
    return {min_x, max_x, min_y, max_y, mean_surface_z};
}

double calculateGSD(const MeasurementGraph &graph, const std::vector<size_t> &node_indices, double mean_surface_z, bool thumbnail)
{
    double arc_per_pixel = 0, mean_camera_z = 0;
    size_t count = 0;
    for (size_t i : node_indices)
    {
        const image &payload = graph.nodes()[i].payload;
        const double h = 0.001;
        const double r0[3] = {0, 0, 1}, r1[3] = {h, 0, 1};
        double pixel[2], shift[2];
        image_from_3d(r0, *payload.model, pixel);
        image_from_3d(r1, *payload.model, shift);
        const double dx = pixel[0] - shift[0], dy = pixel[1] - shift[1];
        double arc_pixel = h / std::sqrt(dx * dx + dy * dy);
        if (thumbnail && payload.model->pixels_rows > 0)
        {
            const double thumb_scale = static_cast<double>(payload.thumbnail_rows) / payload.model->pixels_rows;
            arc_pixel = arc_pixel / thumb_scale;
        }
        // the reference's running means, in node order
        arc_per_pixel = (arc_per_pixel * count + arc_pixel) / (count + 1);
        mean_camera_z = (mean_camera_z * count + payload.position[2]) / (count + 1);
        count++;
    }
    const double average_camera_elevation = mean_camera_z - mean_surface_z;
    return std::max(std::abs(average_camera_elevation * arc_per_pixel), 0.001);
}

Context prepareContext(const std::vector<const surface_model *> &surfaces, const MeasurementGraph &graph, bool thumbnail)
{
    Context c;
    c.bounds = calculateBoundsAndMeanZ(surfaces);
    for (size_t i = 0; i < graph.size_nodes(); i++)
        if (relax_detail::finite4(graph.nodes()[i].payload.orientation))
            c.involved.push_back(i);
    c.gsd = calculateGSD(graph, c.involved, c.bounds.mean_surface_z, thumbnail);
    size_t count = 0;
    for (size_t i : c.involved)
    {
        c.mean_camera_z = (c.mean_camera_z * count + graph.nodes()[i].payload.position[2]) / (count + 1);
        count++;
    }
    c.average_camera_elevation = c.mean_camera_z - c.bounds.mean_surface_z;
    return c;
}

uint64_t inputPixels(const Context &context, const MeasurementGraph &graph)
{
    uint64_t total = 0;
    for (size_t i : context.involved)
    {
        const CameraModel &m = *graph.nodes()[i].payload.model;
        total += static_cast<uint64_t>(m.pixels_cols) * static_cast<uint64_t>(m.pixels_rows);
    }
    return total;
}

void clampOutputResolution(double &gsd, int &width, int &height, uint64_t total_input_pixels)
{
    const uint64_t output_pixels = static_cast<uint64_t>(width) * static_cast<uint64_t>(height);
    if (output_pixels > total_input_pixels && total_input_pixels > 0)
    {
        const double scale_factor = std::sqrt(static_cast<double>(output_pixels) / total_input_pixels);
        gsd *= scale_factor;
        width = static_cast<int>(width / scale_factor);
        height = static_cast<int>(height / scale_factor);
    }
}

void clampOutputMegapixels(double &gsd, int &width, int &height, double max_output_megapixels)
{
    if (!std::isfinite(max_output_megapixels) || max_output_megapixels <= 0.0)
        return;
    const uint64_t output_pixels = static_cast<uint64_t>(width) * static_cast<uint64_t>(height);
    const uint64_t max_output_pixels = static_cast<uint64_t>(max_output_megapixels * 1000000.0);
    if (max_output_pixels == 0 || output_pixels <= max_output_pixels)
        return;
    const double scale_factor = std::sqrt(static_cast<double>(output_pixels) / static_cast<double>(max_output_pixels));
    gsd *= scale_factor;
    width = std::max(1, static_cast<int>(width / scale_factor));
    height = std::max(1, static_cast<int>(height / scale_factor));
}

Plan thumbnailPlan(const Context &context, const MeasurementGraph &graph)
{
    Plan p;
    p.bounds = context.bounds;
    p.gsd = context.gsd;
    p.mean_camera_z = context.mean_camera_z;
    // generateOrthomosaic (ortho.cpp:481-492): the size as a double, guarded, then truncated and clamped
    double image_width = (context.bounds.max_x - context.bounds.min_x) / context.gsd;
    double image_height = (context.bounds.max_y - context.bounds.min_y) / context.gsd;
    if (!std::isfinite(image_width) || image_width < 1)
        image_width = 100;
    if (!std::isfinite(image_height) || image_height < 1)
        image_height = 100;
    p.width = static_cast<int>(image_width);
    p.height = static_cast<int>(image_height);
    clampOutputResolution(p.gsd, p.width, p.height, inputPixels(context, graph));
    return p;
}

Plan dsmPlan(const Context &context, const MeasurementGraph &graph, double max_output_megapixels)
{
    Plan p;
    p.bounds = context.bounds;
    p.gsd = context.gsd;
    p.mean_camera_z = context.mean_camera_z;
    // generateDSMGeoTIFF (ortho.cpp:885-894): truncated first, then guarded, then both clamps
    p.width = static_cast<int>((context.bounds.max_x - context.bounds.min_x) / context.gsd);
    p.height = static_cast<int>((context.bounds.max_y - context.bounds.min_y) / context.gsd);
    if (p.width <= 0)
        p.width = 100;
    if (p.height <= 0)
        p.height = 100;
    clampOutputResolution(p.gsd, p.width, p.height, inputPixels(context, graph));
    clampOutputMegapixels(p.gsd, p.width, p.height, max_output_megapixels);
    return p;
}

TriangleTable triangleTable(const std::vector<const surface_model *> &surfaces)
{
    TriangleTable t;
    for (const surface_model *s : surfaces)
    {
        const MeshGraph &m = s->mesh;
        std::vector<std::array<size_t, 3>> tris;
        for (const MeshEdge &e : m.edges)
        {
            if (e.source == MeshEdge::NONE || e.source >= m.nodes.size() || e.dest >= m.nodes.size())
                continue;
            for (size_t o : e.triangleOppositeNodes)
                if (o != MeshEdge::NONE && o < m.nodes.size() && o != e.source && o != e.dest)
                {
                    std::array<size_t, 3> n{e.source, e.dest, o};
                    std::sort(n.begin(), n.end());
                    tris.push_back(n);
                }
        }
        std::sort(tris.begin(), tris.end());
        tris.erase(std::unique(tris.begin(), tris.end()), tris.end());
        for (const auto &n : tris)
        {
            double c9[9];
            corners(m, n, c9);
            t.tri9.insert(t.tri9.end(), c9, c9 + 9);
            t.nodes.push_back(n);
        }
        t.tri_off.push_back(t.nodes.size());
    }
    return t;
}

namespace
{

// one row of the walkers of the reference's per-pixel loop (a fresh set per row)
struct RowWalkers
{
    const std::vector<const surface_model *> &surfaces;
    std::vector<TriangleWalker> walkers;
    std::vector<size_t> surface_of;
    std::vector<bool> last_hit;
    explicit RowWalkers(const std::vector<const surface_model *> &s) : surfaces(s)
    {
        for (size_t i = 0; i < s.size(); i++)
        {
            TriangleWalker w;
            if (w.init(s[i]->mesh))
            {
                walkers.push_back(w);
                surface_of.push_back(i);
                last_hit.push_back(false);
            }
        }
    }
    // z (NaN: no surface), the surface and its triangle's corners; *capped += walks that ran out of steps
    double height(double x, double y, double mean_camera_z, size_t *surface, std::array<size_t, 3> *tri, uint64_t *capped)
    {
        for (size_t k = 0; k < walkers.size(); k++)
        {
            TriangleWalker &w = walkers[k];
            const MeshGraph &mesh = surfaces[surface_of[k]]->mesh;
            if (!last_hit[k] && !w.init(mesh)) // reinit after anything but an intersection
                continue;
            const bool hit = w.find(relax_detail::v3{0, 0, -1}, relax_detail::v3{x, y, mean_camera_z}) == TriangleWalker::INTERSECTION;
            last_hit[k] = hit;
            if (w.steps > 100)
                ++*capped;
            if (!hit)
                continue;
            std::array<size_t, 3> n{w.tri[0], w.tri[1], w.tri[2]};
            std::sort(n.begin(), n.end());
            double c9[9], z;
            corners(mesh, n, c9);
            if (!ochip_og::triangle_height(c9, x, y, mean_camera_z, &z, false))
                z = w.hit.z; // a plane the canonical order finds parallel: the walker's own height
            *surface = surface_of[k];
            *tri = n;
            return z;
        }
        return NAN;
    }
};

} // namespace

double rayTraceHeight(double x, double y, double mean_camera_z, const std::vector<const surface_model *> &surfaces)
{
    RowWalkers w(surfaces);
    size_t s;
    std::array<size_t, 3> tri;
    uint64_t capped = 0;
    return w.height(x, y, mean_camera_z, &s, &tri, &capped);
}

uint64_t heightsCPU(const std::vector<const surface_model *> &surfaces, const Plan &plan, int64_t row0, int64_t rows,
                    double *z, uint32_t *tri, const TriangleTable *table)
{
    uint64_t capped = 0;
    const int width = plan.width;
#pragma omp parallel for schedule(dynamic) reduction(+ : capped)
    for (int64_t r = 0; r < rows; r++)
    {
        RowWalkers walkers(surfaces);
        const int64_t row = row0 + r;
        for (int col = 0; col < width; col++)
        {
            const double x = col * plan.gsd + plan.bounds.min_x;
            const double y = plan.bounds.max_y - row * plan.gsd;
            size_t s = 0;
            std::array<size_t, 3> n{};
            const double h = walkers.height(x, y, plan.mean_camera_z, &s, &n, &capped);
            const size_t i = (size_t)r * width + col;
            z[i] = h;
            if (tri)
            {
                tri[i] = MISS;
                if (!std::isnan(h) && table)
                {
                    const auto b = table->nodes.begin() + table->tri_off[s], e = table->nodes.begin() + table->tri_off[s + 1];
                    const auto it = std::lower_bound(b, e, n);
                    if (it != e && *it == n)
                        tri[i] = (uint32_t)(it - table->nodes.begin());
                }
            }
        }
    }
    return capped;
}

bool cameras(const Context &context, const MeasurementGraph &graph, Cameras *out, std::string *error)
{
    *out = Cameras{};
    for (size_t i : context.involved)
    {
        const MeasurementGraph::Node &node = graph.nodes()[i];
        const image &p = node.payload;
        if (p.thumbnail_rows == 0 || p.thumbnail_cols == 0)
        {
            *error = "node " + std::to_string(node.id) + " has no thumbnail (och_graph_set_thumbnail)";
            return false;
        }
        // orientation.inverse().toRotationMatrix(): the conjugate over the squared norm
        const double *q = p.orientation;
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        const double qi[4] = {-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2};
        double R[3][3];
        relax_detail::to_matrix(qi, R);
        const CameraModel &m = *p.model;
        double c[24] = {p.position[0], p.position[1], p.position[2]};
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++)
                c[3 + 3 * r + k] = R[r][k];
        const double model[8] = {m.focal_length_pixels, m.principle_point[0], m.principle_point[1], m.radial_distortion[0],
                                 m.radial_distortion[1], m.radial_distortion[2], m.tangential_distortion[0],
                                 m.tangential_distortion[1]};
        std::copy(model, model + 8, c + 12);
        c[20] = m.pixels_rows > 0 ? static_cast<double>(p.thumbnail_rows) / m.pixels_rows : 1.0;
        c[21] = (double)p.thumbnail_rows;
        c[22] = (double)p.thumbnail_cols;
        c[23] = 0;
        out->cams24.insert(out->cams24.end(), c, c + 24);
        out->models.push_back(m);
        out->ids.push_back((uint32_t)(node.id & 0xFFFFFFFFu));
        out->thumb_off.push_back(out->thumbs.size());
        out->thumbs.insert(out->thumbs.end(), p.thumbnail_pixels.begin(), p.thumbnail_pixels.end());
    }
    return true;
}

void colourCPU(const Plan &plan, const Cameras &cams, const double *z, uint8_t *rgba, uint32_t *ids)
{
    const size_t n_cams = cams.ids.size();
#pragma omp parallel for schedule(dynamic)
    for (int row = 0; row < plan.height; row++)
        for (int col = 0; col < plan.width; col++)
        {
            const size_t o = (size_t)row * plan.width + col;
            const double x = col * plan.gsd + plan.bounds.min_x;
            const double y = plan.bounds.max_y - row * plan.gsd;
            uint8_t *px = rgba + 4 * o;
            px[0] = px[1] = px[2] = px[3] = 0; // no surface under the pixel (the reference leaves it unset)
            ids[o] = MISS;
            if (std::isnan(z[o]))
                continue;
            double bd[ochip_og::KNN];
            uint32_t bi[ochip_og::KNN];
            ochip_og::knn_brute(cams.cams24.data(), 24, n_cams, x, y, MISS, bd, bi);
            for (int k = 0; k < ochip_og::KNN && bi[k] != MISS; k++)
            {
                const double *c = &cams.cams24[24 * (size_t)bi[k]];
                // ortho.cpp:590-611 with the host's own image_from_3d (the device restates it: ortho.hip)
                double ray[3], pixel[2];
                if (ochip_og::camera_ray_z(c, x, y, z[o], ray) <= 0)
                    continue;
                image_from_3d(ray, cams.models[bi[k]], pixel);
                int tc, tr;
                if (!ochip_og::thumbnail_cell(c, pixel, &tc, &tr))
                    continue;
                const uint8_t *s = &cams.thumbs[cams.thumb_off[bi[k]] + ((size_t)tr * (size_t)c[22] + tc) * 3];
                px[0] = s[0], px[1] = s[1], px[2] = s[2], px[3] = 255;
                ids[o] = cams.ids[bi[k]];
                break;
            }
            if (ids[o] == MISS) // background checkerboard
            {
                const uint8_t grey = (row + col) % 2 == 0 ? 64 : 128;
                px[0] = px[1] = px[2] = grey;
                px[3] = 0;
            }
        }
}

} // namespace ortho
} // namespace opencalibration_amd
