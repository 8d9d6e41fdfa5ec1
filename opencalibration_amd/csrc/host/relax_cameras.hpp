// The parts of the relax host assembly that every flavour shares and that call nothing on the device: the camera table of
// nodeid2poseopt, the bootstrap plane, and the packing of plane edges into the device's records.  Only types.hpp and
// relax.hpp (the ochip_* record types, no calls), so a stand-alone program can use them without the device library
// (tests/relax_cameras_driver.cpp).  The users: relax.cpp (ground plane and the resident chain), relax_mesh.cpp,
// relax_points.cpp, relax_relative.cpp, and relax_util.hpp's device_filter.
#pragma once

#include "relax.hpp"
#include "types.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace opencalibration_amd
{
namespace relax_detail
{
inline bool finite4(const double *q)
{
    return std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]) && std::isfinite(q[3]);
}
inline bool finite3(const double *p)
{
    return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
}

struct pose_ref // OptimizationPackage::PoseOpt (relax_problem.cpp:182-232)
{
    bool optimize = false;
    const double *loc = nullptr;
    const double *rot = nullptr;
    uint32_t cam = 0; // index into the device camera table
};

// The device's camera table of one problem: the optimised poses first, in the pose list's order, then the context cameras
// in the order of their first use.  A node that appears twice in the pose list (RelaxGroup::init appends the first ring of
// context cameras once per round, relax_group.cpp:40-66) is optimised through its FIRST pose only: _nodes_to_optimize.emplace
// keeps the first (relax_problem.cpp:150-154); the other pose is never touched.
class camera_table
{
  public:
    camera_table(const MeasurementGraph &graph, std::vector<NodePose> &poses)
        : pose_cam(poses.size(), UINT32_MAX), _graph(graph), _poses(poses)
    {
        for (size_t i = 0; i < poses.size(); i++)
            if (_first_pose.emplace(poses[i].node_id, i).second)
            {
                pose_cam[i] = (uint32_t)optimize.size();
                push_camera(poses[i].position, poses[i].orientation, true);
            }
        _n_optimised = optimize.size();
    }

    // nodeid2poseopt (relax_problem.cpp:182-232).  An optimised node: its first pose's own arrays, whatever they hold.  A
    // context node - in the graph, with a finite position and orientation - gets a constant camera on its first use.
    // Anything else: loc == nullptr, and the table stays as it is.
    // Appends to the table, so it is not for OpenMP regions: every caller looks its edges up before it goes parallel.
    pose_ref lookup(size_t node_id)
    {
        pose_ref po;
        auto it = _first_pose.find(node_id);
        if (it != _first_pose.end())
        {
            po.optimize = true;
            po.loc = _poses[it->second].position;
            po.rot = _poses[it->second].orientation;
            po.cam = pose_cam[it->second];
            return po;
        }
        const MeasurementGraph::Node *node = _graph.getNode(node_id);
        if (node != nullptr && finite4(node->payload.orientation) && finite3(node->payload.position))
        {
            po.loc = node->payload.position;
            po.rot = node->payload.orientation;
            auto c = _context_cam.find(node_id);
            if (c == _context_cam.end())
            {
                c = _context_cam.emplace(node_id, (uint32_t)optimize.size()).first;
                push_camera(po.loc, po.rot, false);
            }
            po.cam = c->second;
        }
        return po;
    }

    const std::vector<NodePose> &poses() const // the caller's list
    {
        return _poses;
    }
    size_t size() const // optimised + context cameras so far
    {
        return optimize.size();
    }
    size_t n_optimised() const // the first poses alone: the cameras in front of every context camera
    {
        return _n_optimised;
    }

    // p.second->orientation.normalize() (relax_problem.cpp:1410-1413): q, 4 per camera as the device returns them, into
    // the first poses; a later pose of the same node keeps what it holds
    void store_orientations(const double *q)
    {
        for (size_t i = 0; i < _poses.size(); i++)
        {
            if (pose_cam[i] == UINT32_MAX)
                continue;
            const double *s4 = q + 4 * (size_t)pose_cam[i];
            const double n = std::sqrt(s4[0] * s4[0] + s4[1] * s4[1] + s4[2] * s4[2] + s4[3] * s4[3]);
            for (int k = 0; k < 4; k++)
                _poses[i].orientation[k] = s4[k] / n;
        }
    }

    std::vector<double> pos, q;     // 3 and 4 per camera
    std::vector<uint8_t> optimize;  // 1: a first pose, 0: a context camera
    std::vector<uint32_t> pose_cam; // per pose: its camera, or UINT32_MAX for a later pose of the same node

  private:
    void push_camera(const double *p, const double *r, bool opt)
    {
        pos.insert(pos.end(), p, p + 3);
        q.insert(q.end(), r, r + 4);
        optimize.push_back(opt ? 1 : 0);
    }
    const MeasurementGraph &_graph;
    std::vector<NodePose> &_poses;
    std::unordered_map<size_t, size_t> _first_pose;     // node id -> index of its first pose
    std::unordered_map<size_t, uint32_t> _context_cam; // node id -> camera, for the context cameras
    size_t _n_optimised = 0;
};

// initializeGroundPlane (relax_problem.cpp:1189-1242) + the searcher's orientation fix-up of the single triangle
// (MeshIntersectionSearcher::triangleIntersect, src/surface/intersect.cpp:56-163), for a list of camera positions: the
// corners in the searcher's order (corner_of[i]: which corner of the surface model stands at place i) and the start height
inline void bootstrap_plane(const std::vector<const double *> &positions, double tri_xy[6], double *z0, int corner_of[3] = nullptr)
{
    double lo[2] = {1e12, 1e12}, hi[2] = {-1e12, -1e12}, height = 0;
    for (const double *p : positions)
    {
        for (int a = 0; a < 2; a++)
        {
            lo[a] = std::min(lo[a], p[a]);
            hi[a] = std::max(hi[a], p[a]);
        }
        height += p[2];
    }
    height /= (double)positions.size();
    const double margin = 50;
    height -= margin;
    const double cx = (lo[0] + hi[0]) / 2, cy = (lo[1] + hi[1]) / 2;
    const double spacing = std::max(hi[0] - lo[0], hi[1] - lo[1]) + margin;
    const double c[3][2] = {{-spacing + cx, -spacing + cy}, {spacing + cx, -spacing + cy}, {0 + cx, spacing + cy}};
    int tri[3] = {0, 1, 2};
    if ((c[1][0] - c[0][0]) * (c[2][1] - c[0][1]) - (c[1][1] - c[0][1]) * (c[2][0] - c[0][0]) < 0) // anticlockwise(a, b, c)
        std::swap(tri[0], tri[1]);
    for (int i = 0; i < 3; i++)
    {
        tri_xy[2 * i] = c[tri[i]][0];
        tri_xy[2 * i + 1] = c[tri[i]][1];
        if (corner_of)
            corner_of[i] = tri[i];
    }
    *z0 = height;
}

// the descriptor term of a match's score (gridFilterMatchesPerImage, relax_problem.cpp:234-309): an inlier that names no match counts as a perfect one
inline double descriptor_score(const camera_relations &rel, const feature_match_denormalized &m)
{
    return m.match_index < rel.matches.size() ? 1.0 - rel.matches[m.match_index].distance : 1.0;
}

// The edges of a plane set-up or a chain as the device takes them (ochip_plane_setup_create, ochip_plane_chain_create):
// one ochip_plane_edge per edge with its cameras, its two lens models - rows of models10, numbered by first appearance -
// and where its inlier matches start in the one array of ochip_plane_inlier records that pack_inliers fills.
struct plane_edge_packer
{
    std::vector<ochip_plane_edge> pe;
    std::vector<const MeasurementGraph::Edge *> edge;
    std::vector<double> models10; // focal, principal point, 3 radial, 2 tangential, columns, rows
    uint64_t n_inliers = 0;

    uint32_t n_models() const
    {
        return (uint32_t)_model_index.size();
    }
    void add(const MeasurementGraph &graph, const MeasurementGraph::Edge &e, uint32_t cam_a, uint32_t cam_b)
    {
        const camera_relations &rel = e.payload;
        ochip_plane_edge r{};
        r.cam_a = cam_a;
        r.cam_b = cam_b;
        r.model_a = model_of(graph.getNode(e.source)->payload.model.get());
        r.model_b = model_of(graph.getNode(e.dest)->payload.model.get());
        r.n_inliers = (uint32_t)rel.inlier_matches.size();
        r.flags = rel.relationType == camera_relations::RelationType::HOMOGRAPHY ? 1u : 0u;
        r.inlier_offset = n_inliers;
        std::memcpy(r.H, rel.ransac_relation, sizeof r.H);
        n_inliers += r.n_inliers;
        pe.push_back(r);
        edge.push_back(&e);
    }
    // dst: room for n_inliers records (40 bytes each)
    void pack_inliers(ochip_plane_inlier *dst) const
    {
#pragma omp parallel for schedule(dynamic, 16)
        for (size_t j = 0; j < pe.size(); j++)
        {
            const camera_relations &rel = edge[j]->payload;
            ochip_plane_inlier *o = dst + pe[j].inlier_offset;
            for (size_t idx = 0; idx < rel.inlier_matches.size(); idx++)
            {
                const feature_match_denormalized &m = rel.inlier_matches[idx];
                o[idx].px1[0] = m.pixel_1[0], o[idx].px1[1] = m.pixel_1[1];
                o[idx].px2[0] = m.pixel_2[0], o[idx].px2[1] = m.pixel_2[1];
                o[idx].descriptor_score = descriptor_score(rel, m);
            }
        }
    }

  private:
    uint32_t model_of(const CameraModel *m)
    {
        auto it = _model_index.find(m);
        if (it != _model_index.end())
            return it->second;
        const double row[10] = {m->focal_length_pixels,  m->principle_point[0],   m->principle_point[1],       m->radial_distortion[0],
                                m->radial_distortion[1], m->radial_distortion[2], m->tangential_distortion[0], m->tangential_distortion[1],
                                (double)m->pixels_cols,  (double)m->pixels_rows};
        models10.insert(models10.end(), row, row + 10);
        return _model_index.emplace(m, (uint32_t)_model_index.size()).first->second;
    }
    std::unordered_map<const CameraModel *, uint32_t> _model_index;
};

} // namespace relax_detail
} // namespace opencalibration_amd
