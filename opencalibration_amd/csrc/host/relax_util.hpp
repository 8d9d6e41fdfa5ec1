// Helpers shared by the host assembly of the five relax set-ups: relax.cpp (the ground plane on the pair-record engine and
// the resident chain in front of it), relax_mesh.cpp (mesh / tracks / intrinsics on the general engine), relax_points.cpp
// (3-D points) and relax_relative.cpp (homography decompositions).  What needs no device call - the camera table, the
// bootstrap plane, the packing of plane edges - is in relax_cameras.hpp; here: small vector algebra, the host's grid filter,
// the device's grid filter, the lens block of the descriptors and what follows every device solve.
#pragma once

#include "ransac.hpp" // image_to_3d
#include "relax_cameras.hpp"
#include "relax_mesh.hpp" // the OPT_* bits

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace opencalibration_amd
{
namespace relax_detail
{
using clk = std::chrono::steady_clock;
inline double since(clk::time_point t0)
{
    return std::chrono::duration<double>(clk::now() - t0).count();
}

struct v3
{
    double x, y, z;
};
inline v3 sub(const v3 &a, const v3 &b)
{
    return {a.x - b.x, a.y - b.y, a.z - b.z};
}
inline v3 add(const v3 &a, const v3 &b)
{
    return {a.x + b.x, a.y + b.y, a.z + b.z};
}
inline v3 mul(const v3 &a, double s)
{
    return {a.x * s, a.y * s, a.z * s};
}
inline double dot(const v3 &a, const v3 &b)
{
    return a.x * b.x + a.y * b.y + a.z * b.z;
}
inline v3 cross(const v3 &a, const v3 &b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
inline bool hasnan4(const double *q)
{
    return std::isnan(q[0]) || std::isnan(q[1]) || std::isnan(q[2]) || std::isnan(q[3]);
}

// Eigen::Quaternion::toRotationMatrix
inline void to_matrix(const double *q, double R[3][3])
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0][0] = 1 - (tyy + tzz), R[0][1] = txy - twz, R[0][2] = txz + twy;
    R[1][0] = txy + twz, R[1][1] = 1 - (txx + tzz), R[1][2] = tyz - twx;
    R[2][0] = txz - twy, R[2][1] = tyz + twx, R[2][2] = 1 - (txx + tyy);
}
inline v3 apply(const double R[3][3], const v3 &v)
{
    return {R[0][0] * v.x + R[0][1] * v.y + R[0][2] * v.z, R[1][0] * v.x + R[1][1] * v.y + R[1][2] * v.z,
            R[2][0] * v.x + R[2][1] * v.y + R[2][2] * v.z};
}
// Eigen QuaternionBase::_transformVector
inline v3 rotate(const double *q, const v3 &v)
{
    const v3 qv{q[0], q[1], q[2]};
    v3 uv = cross(qv, v);
    uv = add(uv, uv);
    return add(add(v, mul(uv, q[3])), cross(qv, uv));
}

// src/geometry/intersection.cpp:116-143: midpoint of closest approach, signed squared gap
inline void ray_intersection(const v3 &d1, const v3 &o1, const v3 &d2, const v3 &o2, v3 *mid, double *err)
{
    *mid = {NAN, NAN, NAN};
    *err = NAN;
    const double n11 = dot(d1, d1), n12 = dot(d1, d2), n22 = dot(d2, d2);
    const double denom = n11 * n22 - n12 * n12;
    if (std::abs(denom) > 1e-9)
    {
        const v3 off = sub(o1, o2);
        const double od1 = dot(off, d1), od2 = dot(off, d2);
        const double t = (n12 * od2 - n22 * od1) / denom;
        const double s = (n11 * od2 - n12 * od1) / denom;
        const v3 p1 = add(o1, mul(d1, t)), p2 = add(o2, mul(d2, s));
        *mid = mul(add(p1, p2), 0.5);
        const v3 g = sub(p1, p2);
        *err = dot(g, g) * (t >= 0 && s >= 0 ? 1 : -1);
    }
}

// after every device solve: what the caller's timers take from the summary
inline void note_solve(RelaxTimers *t, const ochip_relax_summary &s)
{
    if (t == nullptr)
        return;
    t->solves++;
    t->iterations_total += s.iterations;
    t->last_iterations = s.iterations;
    t->last_initial_cost = s.initial_cost;
    t->last_final_cost = s.final_cost;
    t->last_residual_blocks = s.num_residual_blocks;
}

// a device call failed: its name and the context's text into *error (which may be null); returns false
inline bool device_fail(ochip_ctx *ctx, std::string *error, const char *what)
{
    if (error)
        *error = std::string(what) + ": " + ochip_last_error(ctx);
    return false;
}

// The lens block of a descriptor: the 8 doubles of a forward or an inverse model ...
template <typename Model> void pack_model8(const Model &m, double out[8])
{
    out[0] = m.focal_length_pixels;
    out[1] = m.principle_point[0], out[2] = m.principle_point[1];
    for (int i = 0; i < 3; i++)
        out[3 + i] = m.radial_distortion[i];
    out[6] = m.tangential_distortion[0], out[7] = m.tangential_distortion[1];
}
// ... and the SubsetManifold of its radial block (relax_problem.cpp:533-556, :1160-1180): Brown k1 / k1 k2 / k1 k2 k3 free.
// With no parameterisation chosen - also when LENS_DISTORTIONS_RADIAL is not among the options at all - the block stays a
// free Euclidean one.
inline int radial_free_count(uint32_t options)
{
    if ((options & OPT_LENS_DISTORTIONS_RADIAL) && !(options & OPT_LENS_DISTORTIONS_RADIAL_BROWN246_PARAMETERIZATION))
    {
        if (options & OPT_LENS_DISTORTIONS_RADIAL_BROWN24_PARAMETERIZATION)
            return 2;
        if (options & OPT_LENS_DISTORTIONS_RADIAL_BROWN2_PARAMETERIZATION)
            return 1;
    }
    return 3;
}

// page-locked staging from the context's pool: no first-touch faults on ~40 bytes x every inlier of a survey, and the
// upload runs at the link rate
struct host_staging
{
    ochip_ctx *ctx;
    void *p = nullptr;
    explicit host_staging(ochip_ctx *c) : ctx(c)
    {
    }
    host_staging(const host_staging &) = delete;
    host_staging &operator=(const host_staging &) = delete;
    ~host_staging()
    {
        if (p)
            ochip_host_free(ctx, p);
    }
    bool alloc(size_t bytes, std::string *error)
    {
        return ochip_host_alloc(ctx, bytes, &p) == OCHIP_OK || device_fail(ctx, error, "ochip_host_alloc");
    }
};


// Scores of gridFilterMatchesPerImage + GridFilter::addMeasurement (grid_filter.hpp:33-51): the
// measurements arrive best-first, so the first one in a cell stays.  Returns per inlier: bit0 = on the
// source whitelist, bit1 = on the dest whitelist.
inline std::vector<uint8_t> grid_filter(const MeasurementGraph &_graph, const MeasurementGraph::Edge &edge, const pose_ref &s,
                                    const pose_ref &d, double res)
{
    const camera_relations &rel = edge.payload;
    const CameraModel &sm = *_graph.getNode(edge.source)->payload.model, &dm = *_graph.getNode(edge.dest)->payload.model;
    double Rs[3][3], Rd[3][3];
    to_matrix(s.rot, Rs);
    to_matrix(d.rot, Rd);
    const v3 so{s.loc[0], s.loc[1], s.loc[2]}, d_o{d.loc[0], d.loc[1], d.loc[2]};
    std::vector<std::pair<double, size_t>> scored;
    scored.reserve(rel.inlier_matches.size());
    for (size_t idx = 0; idx < rel.inlier_matches.size(); idx++)
    {
        const feature_match_denormalized &m = rel.inlier_matches[idx];
        double r1[3], r2[3];
        image_to_3d(m.pixel_1, sm, r1);
        image_to_3d(m.pixel_2, dm, r2);
        const v3 sd = apply(Rs, v3{r1[0], r1[1], r1[2]}), dd = apply(Rd, v3{r2[0], r2[1], r2[2]});
        v3 mid;
        double gap;
        ray_intersection(sd, so, dd, d_o, &mid, &gap);
        const double intersection_score = gap < 0 ? 0. : 1. / (1. + gap);
        const double cos_angle = dot(sd, dd);
        const double angle_score = 1.0 - cos_angle * cos_angle;
        double ransac_score = 1.0;
        if (rel.relationType == camera_relations::RelationType::HOMOGRAPHY)
        {
            const double sx = (m.pixel_1[0] - sm.principle_point[0]) / sm.focal_length_pixels;
            const double sy = (m.pixel_1[1] - sm.principle_point[1]) / sm.focal_length_pixels;
            const double dx = (m.pixel_2[0] - dm.principle_point[0]) / dm.focal_length_pixels;
            const double dy = (m.pixel_2[1] - dm.principle_point[1]) / dm.focal_length_pixels;
            const double *H = rel.ransac_relation;
            const double hx = H[0] * sx + H[1] * sy + H[2] * 1.0, hy = H[3] * sx + H[4] * sy + H[5] * 1.0,
                         hz = H[6] * sx + H[7] * sy + H[8] * 1.0;
            const double ex = dx - hx / hz, ey = dy - hy / hz;
            ransac_score = 1.0 / (1.0 + std::sqrt(ex * ex + ey * ey));
        }
        scored.emplace_back(intersection_score * angle_score * descriptor_score(rel, m) * ransac_score, idx);
    }
    std::vector<uint8_t> keep(rel.inlier_matches.size(), 0);
    auto cell = [res](double x, double y, int *cx, int *cy) {
        *cx = (int)std::floor(x / res);
        *cy = (int)std::floor(y / res);
    };
    // GridFilter::addMeasurement keeps, per cell of each image, the first measurement in descending score order,
    // i.e. the best-scoring one.  That needs no sort unless two candidates for a cell's best tie exactly (the
    // unstable std::sort then decides): one pass over a small dense cell table, and the sorted walk only as the
    // fall-back for ties or cells outside the table.
    constexpr int G = 48; // cells per axis the table covers (pixels / image size lies in [0, 1): 1 / 0.15 < 7; a mesh run at grid fraction 0.025 has 40)
    int best_s[G * G], best_d[G * G];
    std::fill(best_s, best_s + G * G, -1);
    std::fill(best_d, best_d + G * G, -1);
    bool exact = true;
    for (size_t k = 0; k < scored.size() && exact; k++)
    {
        const double score = scored[k].first;
        if (!(score > 0))
            continue;
        const feature_match_denormalized &m = rel.inlier_matches[scored[k].second];
        int cx, cy, dx, dy;
        cell(m.pixel_1[0] / sm.pixels_cols, m.pixel_1[1] / sm.pixels_rows, &cx, &cy);
        cell(m.pixel_2[0] / dm.pixels_cols, m.pixel_2[1] / dm.pixels_rows, &dx, &dy);
        if (cx < 0 || cy < 0 || cx >= G || cy >= G || dx < 0 || dy < 0 || dx >= G || dy >= G)
        {
            exact = false;
            break;
        }
        int &bs = best_s[cx * G + cy], &bd = best_d[dx * G + dy];
        if (bs < 0 || score > scored[bs].first)
            bs = (int)k;
        else if (score == scored[bs].first)
            exact = false;
        if (bd < 0 || score > scored[bd].first)
            bd = (int)k;
        else if (score == scored[bd].first)
            exact = false;
    }
    if (exact)
    {
        for (int c = 0; c < G * G; c++)
        {
            if (best_s[c] >= 0)
                keep[scored[best_s[c]].second] |= 1;
            if (best_d[c] >= 0)
                keep[scored[best_d[c]].second] |= 2;
        }
        return keep;
    }
    std::fill(keep.begin(), keep.end(), 0);
    std::sort(scored.begin(), scored.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::unordered_map<uint64_t, char> scell, dcell;
    auto key = [res](double x, double y) {
        return (static_cast<uint64_t>((int)std::floor(x / res)) << 32) | static_cast<uint32_t>((int)std::floor(y / res));
    };
    for (const auto &[score, idx] : scored)
    {
        if (!(score > 0))
            continue;
        const feature_match_denormalized &m = rel.inlier_matches[idx];
        if (scell.emplace(key(m.pixel_1[0] / sm.pixels_cols, m.pixel_1[1] / sm.pixels_rows), 1).second)
            keep[idx] |= 1;
        if (dcell.emplace(key(m.pixel_2[0] / dm.pixels_cols, m.pixel_2[1] / dm.pixels_rows), 1).second)
            keep[idx] |= 2;
    }
    return keep;
}


// gridFilterMatchesPerImage (relax_problem.cpp:234-309) of a list of edges on the device (ochip_plane_setup_create,
// csrc/relax_setup.hip): the edges' inlier matches are packed into page-locked staging (40 bytes each), one wavefront per
// edge scores and filters them, and the edges the device only flags - two matches sharing a cell's best score, which the
// reference's unstable std::sort decides, or a match outside the cell table - are decided by grid_filter above.
// keep: the edges' flags back to back (edge j's start at pk.pe[j].inlier_offset).  The handle stays open for the caller
// (the ground-plane set-up goes on to ochip_plane_setup_blocks); destroy it with ochip_plane_setup_destroy.
struct device_filter
{
    plane_edge_packer pk; // the edges that went in, in order
    std::vector<pose_ref> src, dst;
    std::vector<uint8_t> keep;
    ochip_plane_setup *handle = nullptr;
    double seconds_pack = 0;
    ~device_filter()
    {
        if (handle)
            ochip_plane_setup_destroy(handle);
    }
    // edges[k] with poses src[k] / dst[k]; nullptr entries are skipped.  triangle: the plane's border triangle (only the
    // block list uses it).  Returns false with *error set when a device call fails.
    bool run(ochip_ctx *ctx, const MeasurementGraph &graph, const std::vector<const MeasurementGraph::Edge *> &edges,
             const std::vector<pose_ref> &srcs, const std::vector<pose_ref> &dsts, size_t n_edges, const camera_table &cams,
             const double triangle_xy6[6], double fraction, std::string *error)
    {
        const auto t0 = clk::now();
        for (size_t k = 0; k < n_edges; k++)
        {
            if (edges[k] == nullptr)
                continue;
            pk.add(graph, *edges[k], srcs[k].cam, dsts[k].cam);
            src.push_back(srcs[k]);
            dst.push_back(dsts[k]);
        }
        host_staging inl(ctx);
        if (!inl.alloc((pk.n_inliers ? pk.n_inliers : 1) * sizeof(ochip_plane_inlier), error))
            return false;
        ochip_plane_inlier *const rec = static_cast<ochip_plane_inlier *>(inl.p);
        pk.pack_inliers(rec);
        seconds_pack = since(t0);
        keep.assign(pk.n_inliers, 0);
        std::vector<uint8_t> inexact(pk.pe.size());
        if (ochip_plane_setup_create(ctx, pk.pe.data(), (uint32_t)pk.pe.size(), rec, pk.n_inliers, cams.pos.data(), cams.q.data(),
                                     (uint32_t)cams.size(), pk.models10.data(), pk.n_models(), triangle_xy6, fraction, keep.data(),
                                     inexact.data(), &handle) != OCHIP_OK)
            return device_fail(ctx, error, "ochip_plane_setup_create");
        for (size_t j = 0; j < pk.pe.size(); j++)
            if (inexact[j])
            {
                const std::vector<uint8_t> k8 = grid_filter(graph, *pk.edge[j], src[j], dst[j], fraction);
                std::copy(k8.begin(), k8.end(), keep.begin() + pk.pe[j].inlier_offset);
                if (ochip_plane_setup_override(handle, pk.pe[j].inlier_offset, k8.size(), k8.data()) != OCHIP_OK)
                    return device_fail(ctx, error, "ochip_plane_setup_override");
            }
        return true;
    }
};

} // namespace relax_detail
} // namespace opencalibration_amd
