// runRelativeOrientation (src/relax/relax.cpp:14-42) on the device: setupDecompositionProblem (src/relax/relax_problem.cpp:
// 40-59) - one MultiDecomposedRotationCost block per whitelisted edge with inliers (addRelationCost, :311-350), HuberLoss of
// 10 degrees, the downward prior on every optimised camera (:1290-1301), initial trust-region radius 0.1 - solved by the
// general engine (ochip_relaxg_*: relation blocks); cameras whose orientation is NaN are initialised one at a time, each
// followed by a solve of the whole problem (relax.cpp:21-34).
#include "relax_mesh.hpp"

#include "relax_util.hpp"

namespace opencalibration_amd
{

namespace
{
using namespace relax_detail;

bool solve_decomposition_problem(ochip_ctx *ctx, const MeasurementGraph &graph, std::vector<NodePose> &poses,
                                 const std::vector<size_t> &edges_to_optimize, RelaxTimers *timers, std::string *error)
{
    auto t0 = clk::now();
    camera_table cams(graph, poses);
    std::vector<uint32_t> rel_cam;
    std::vector<double> rel_pose;
    std::unordered_map<size_t, char> used;
    for (size_t edge_id : edges_to_optimize)
    {
        const MeasurementGraph::Edge *edge = graph.getEdge(edge_id);
        if (edge == nullptr || used.count(edge_id))
            continue;
        if (edge->payload.inlier_matches.empty()) // addRelationCost (:311-350)
            continue;
        const pose_ref s = cams.lookup(edge->source), d = cams.lookup(edge->dest);
        if (s.loc == nullptr || d.loc == nullptr)
            continue;
        if (!finite4(s.rot) || !finite4(d.rot) || !finite3(s.loc) || !finite3(d.loc))
            continue;
        if (s.cam == d.cam)
            continue; // (an edge from an image to itself carries no relative orientation)
        rel_cam.push_back(s.cam);
        rel_cam.push_back(d.cam);
        for (const decomposed_pose &p : edge->payload.relative_poses)
        {
            rel_pose.insert(rel_pose.end(), p.orientation, p.orientation + 4);
            rel_pose.insert(rel_pose.end(), p.position, p.position + 3);
            rel_pose.push_back((double)p.score);
        }
        used.emplace(edge_id, 1);
    }
    // addDownwardsPrior (:1290-1301)
    std::vector<uint32_t> down_cam;
    for (size_t i = 0; i < poses.size(); i++)
        if (cams.pose_cam[i] != UINT32_MAX && !hasnan4(poses[i].orientation))
            down_cam.push_back(cams.pose_cam[i]);
    if (rel_cam.empty() && down_cam.empty())
        return true; // NumResidualBlocks() == 0
    // a camera whose orientation is not finite cannot be evaluated; Ceres would fail the whole solve on it
    ochip_relaxg_desc d{};
    d.n_cams = (uint32_t)cams.size();
    d.cam_pos = cams.pos.data();
    d.cam_q = cams.q.data();
    d.cam_optimize = cams.optimize.data();
    d.n_down = (uint32_t)down_cam.size();
    d.down_cam = down_cam.data();
    d.down_weight = 1e-3;
    d.n_rel = (uint32_t)(rel_cam.size() / 2);
    d.rel_cam = rel_cam.data();
    d.rel_pose = rel_pose.data();
    d.rel_huber_a = 10 * M_PI / 180; // HuberLoss(10 degrees), :44
    d.huber_a = 1 * M_PI / 180;
    d.model[0] = 1.0;
    d.focal_lo = 100.0;
    d.focal_hi = 20000.0;
    ochip_relaxg_problem *dev = nullptr;
    if (ochip_relaxg_problem_create(ctx, &d, &dev) != OCHIP_OK)
        return device_fail(ctx, error, "ochip_relaxg_problem_create");
    if (timers)
        timers->setup_host += since(t0);
    t0 = clk::now();
    ochip_relax_options o{100, 0.1, 1e-6, 1e-10, 1e-8}; // initial_trust_region_radius = 0.1 (:47)
    ochip_relax_summary s{};
    std::vector<double> q(cams.size() * 4);
    const bool ok = ochip_relaxg_solve(dev, &o, &s) == OCHIP_OK && ochip_relaxg_get_state(dev, q.data(), nullptr, nullptr) == OCHIP_OK;
    if (!ok)
        device_fail(ctx, error, "ochip_relaxg_solve");
    ochip_relaxg_problem_destroy(dev);
    if (timers)
        timers->device += since(t0);
    if (!ok)
        return false;
    note_solve(timers, s);
    cams.store_orientations(q.data()); // orientation.normalize(), :1410-1413
    return true;
}

} // namespace

bool relax_relative_orientation(ochip_ctx *ctx, const MeasurementGraph &graph, std::vector<NodePose> &nodes,
                                const std::vector<size_t> &edges_to_optimize, RelaxTimers *timers, std::string *error)
{
    std::vector<NodePose> backup = nodes;
    // DOWN_ORIENTED_NORTH = Quaterniond(AngleAxisd(M_PI, UnitX)), relax.cpp:12
    const double down[4] = {std::sin(M_PI / 2), 0.0, 0.0, std::cos(M_PI / 2)};
    for (auto &node : nodes)
        if (hasnan4(node.orientation))
        {
            std::memcpy(node.orientation, down, sizeof down);
            if (!solve_decomposition_problem(ctx, graph, nodes, edges_to_optimize, timers, error))
            {
                nodes = backup;
                return false;
            }
        }
    if (!solve_decomposition_problem(ctx, graph, nodes, edges_to_optimize, timers, error))
    {
        nodes = backup;
        return false;
    }
    return true;
}

} // namespace opencalibration_amd
