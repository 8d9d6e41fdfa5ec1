#include "../env.hpp"
#include "relax.hpp"

#include "relax_util.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <memory>
#include <unordered_map>

namespace opencalibration_amd
{

namespace
{
using namespace relax_detail;

std::atomic<int> g_setup_check{0}, g_setup_checked{0};

// One ground-plane problem: host assembly + device solve.
class GroundPlaneProblem
{
  public:
    GroundPlaneProblem(ochip_ctx *ctx, const MeasurementGraph &graph, std::vector<NodePose> &poses)
        : _ctx(ctx), _graph(graph), _cams(graph, poses)
    {
    }
    ~GroundPlaneProblem()
    {
        if (_dev)
            ochip_relax_problem_destroy(_dev);
    }

    // setupGroundPlaneProblem (relax_problem.cpp:61-81)
    bool setup(const std::vector<size_t> &edges_to_optimize, std::string *error, const RelaxShard *shard = nullptr)
    {
        const std::vector<NodePose> &poses = _cams.poses();
        const bool verbose = ochip_verbose("relax");
        auto tmark = clk::now();
        auto lap = [&](const char *what) {
            if (verbose)
                fprintf(stderr, "[relax setup] %-28s %.3f ms\n", what, since(tmark) * 1e3);
            tmark = clk::now();
        };
        // initializeGroundPlane (:1189-1242) under the optimised cameras, its corners in the searcher's order: the
        // searcher's orientation fix-up of the single triangle happens on its first use and is the same for every edge
        {
            std::vector<const double *> positions;
            for (size_t i = 0; i < poses.size(); i++)
                if (_cams.pose_cam[i] != UINT32_MAX)
                    positions.push_back(poses[i].position);
            double z0;
            bootstrap_plane(positions, _tri_xy, &z0, _corner_of);
            _z[0] = _z[1] = _z[2] = z0;
        }

        // gridFilterMatchesPerImage (:234-309): an edge without usable poses stops the whole pass
        size_t n_filter = edges_to_optimize.size();
        std::vector<pose_ref> src(edges_to_optimize.size()), dst(edges_to_optimize.size());
        for (size_t k = 0; k < edges_to_optimize.size(); k++)
        {
            const MeasurementGraph::Edge *e = _graph.getEdge(edges_to_optimize[k]);
            if (e == nullptr)
                continue;
            src[k] = _cams.lookup(e->source);
            dst[k] = _cams.lookup(e->dest);
            if ((src[k].loc == nullptr || dst[k].loc == nullptr) && n_filter == edges_to_optimize.size())
                n_filter = k;
        }
        lap("pose lookup");
        // gridFilterMatchesPerImage (:234-309) and addRayTriangleMeasurementCost (:388-560, fixed intrinsics) on the
        // device: ochip_plane_setup_* (csrc/relax_setup.hip).  Edges past the first one without poses get no filter pass,
        // hence no whitelist and no blocks.
        std::vector<const MeasurementGraph::Edge *> edges(n_filter, nullptr);
        for (size_t k = 0; k < n_filter; k++)
            edges[k] = _graph.getEdge(edges_to_optimize[k]);
        device_filter df;
        if (!df.run(_ctx, _graph, edges, src, dst, n_filter, _cams, _tri_xy, 0.15, error))
            return false;
        ochip_plane_setup *const ps = df.handle;
        lap("grid filter (device)");
        uint64_t total_blocks = 0;
        if (ochip_plane_setup_blocks(ps, nullptr, nullptr, nullptr, 0, &total_blocks) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_plane_setup_blocks");
        _blk_a.resize(total_blocks);
        _blk_b.resize(total_blocks);
        _blk_rays.resize(total_blocks * 6);
        if (ochip_plane_setup_blocks(ps, _blk_a.data(), _blk_b.data(), _blk_rays.data(), total_blocks, &total_blocks) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_plane_setup_blocks");
        lap("edge blocks (device)");
        if (g_setup_check.load())
        {
            // the same two passes with the host code (relax_util.hpp), compared bit for bit
            edge_blocks all;
            for (size_t j = 0; j < df.pk.edge.size(); j++)
                add_edge_blocks(*df.pk.edge[j], df.src[j], df.dst[j], grid_filter(_graph, *df.pk.edge[j], df.src[j], df.dst[j], 0.15), all);
            if (all.a != _blk_a || all.b != _blk_b || all.rays.size() != _blk_rays.size() ||
                std::memcmp(all.rays.data(), _blk_rays.data(), all.rays.size() * sizeof(double)) != 0)
            {
                if (error)
                    *error = "relax set-up: the device's residual blocks differ from the host's (" + std::to_string(_blk_a.size()) + " vs " +
                         std::to_string(all.a.size()) + ")";
                return false;
            }
            g_setup_checked.fetch_add(1);
        }
        // addDownwardsPrior (:1290-1301)
        for (size_t i = 0; i < poses.size(); i++)
            if (_cams.pose_cam[i] != UINT32_MAX && !hasnan4(poses[i].orientation))
                _prior_cam.push_back(_cams.pose_cam[i]);

        lap("concatenate");
        ochip_relax_desc d{};
        d.n_cams = (uint32_t)_cams.size();
        d.cam_pos = _cams.pos.data();
        d.cam_q = _cams.q.data();
        d.cam_optimize = _cams.optimize.data();
        std::memcpy(d.plane_xy, _tri_xy, sizeof _tri_xy);
        for (int i = 0; i < 3; i++)
        {
            d.plane_z[i] = _z[i];
            d.z_optimize[i] = 1;
        }
        d.n_blocks = (uint32_t)_blk_a.size();
        d.blk_cam_a = _blk_a.data();
        d.blk_cam_b = _blk_b.data();
        d.blk_rays = _blk_rays.data();
        d.n_prior = (uint32_t)_prior_cam.size();
        d.prior_cam = _prior_cam.data();
        d.huber_a = 1 * M_PI / 180; // HuberLoss(1 degree), :68
        d.prior_weight = 1e-3;
        if (ochip_relax_problem_create(_ctx, &d, &_dev) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_relax_problem_create");
        if (shard && (shard->world > 1 || shard->exchange) &&
            ochip_relax_set_shard(_dev, shard->rank, shard->world, shard->exchange, shard->user) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_relax_set_shard");
        lap("ochip_relax_problem_create");
        return true;
    }

    // relaxObservedModelOnly (:931-984) then solve (:1390-1420)
    bool relax_observed_model_only(RelaxTimers *t, std::string *error)
    {
        if (ochip_relax_set_cameras_constant(_dev, 1) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_relax_set_cameras_constant");
        const bool ok = solve(t, error);
        if (ochip_relax_set_cameras_constant(_dev, 0) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_relax_set_cameras_constant");
        return ok;
    }

    bool solve(RelaxTimers *t, std::string *error)
    {
        if (_blk_a.empty() && _prior_cam.empty())
            return true; // NumResidualBlocks() == 0: early exit of :1398-1402
        ochip_relax_options o{100, 1.0, 1e-6, 1e-10, 1e-8}; // relax_problem.cpp:30-37 + Ceres defaults
        ochip_relax_summary s{};
        if (ochip_relax_solve(_dev, &o, &s) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_relax_solve");
        note_solve(t, s);
        std::vector<double> q(_cams.size() * 4);
        if (ochip_relax_get_state(_dev, q.data(), _z) != OCHIP_OK)
            return device_fail(_ctx, error, "ochip_relax_get_state");
        _cams.store_orientations(q.data());
        return true;
    }

    void surface(surface_model_plane *out) const
    {
        for (int i = 0; i < 3; i++)
        {
            out->corner[_corner_of[i]][0] = _tri_xy[2 * i];
            out->corner[_corner_of[i]][1] = _tri_xy[2 * i + 1];
            out->corner[_corner_of[i]][2] = _z[i];
        }
    }

  private:
    // MeshIntersectionSearcher::triangleIntersect (src/surface/intersect.cpp:56-163) on the single border triangle: the
    // three edge tests (the set-up check's host path)
    static bool anticlockwise(const double *a, const double *b, const double *c)
    {
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0;
    }
    bool vertical_ray_hits_plane_triangle(double px, double py) const
    {
        const double P[2] = {px, py};
        for (int i = 0; i < 3; i++)
            if (anticlockwise(P, _tri_xy + 2 * i, _tri_xy + 2 * ((i + 1) % 3)))
                return false;
        return true;
    }

    struct edge_blocks
    {
        std::vector<uint32_t> a, b;
        std::vector<double> rays;
    };

    void add_edge_blocks(const MeasurementGraph::Edge &edge, const pose_ref &s, const pose_ref &d,
                         const std::vector<uint8_t> &keep, edge_blocks &out) const
    {
        const camera_relations &rel = edge.payload;
        const CameraModel &sm = *_graph.getNode(edge.source)->payload.model, &dm = *_graph.getNode(edge.dest)->payload.model;
        const v3 so{s.loc[0], s.loc[1], s.loc[2]}, d_o{d.loc[0], d.loc[1], d.loc[2]};
        for (size_t idx = 0; idx < rel.inlier_matches.size(); idx++)
        {
            if (idx >= keep.size() || keep[idx] == 0)
                continue;
            const feature_match_denormalized &m = rel.inlier_matches[idx];
            double r1[3], r2[3];
            image_to_3d(m.pixel_1, sm, r1);
            image_to_3d(m.pixel_2, dm, r2);
            v3 mid;
            double gap;
            ray_intersection(rotate(s.rot, v3{r1[0], r1[1], r1[2]}), so, rotate(d.rot, v3{r2[0], r2[1], r2[2]}), d_o, &mid,
                             &gap);
            if (std::isnan(mid.x) || std::isnan(mid.y))
                continue;
            if (!vertical_ray_hits_plane_triangle(mid.x, mid.y))
                continue;
            out.a.push_back(s.cam);
            out.b.push_back(d.cam);
            out.rays.insert(out.rays.end(), r1, r1 + 3);
            out.rays.insert(out.rays.end(), r2, r2 + 3);
        }
    }

    ochip_ctx *_ctx;
    const MeasurementGraph &_graph;
    camera_table _cams;
    std::vector<double> _blk_rays;
    std::vector<uint32_t> _blk_a, _blk_b, _prior_cam;
    // the plane's triangle in the searcher's order with its heights; corner_of[i]: the surface model's corner at place i
    double _tri_xy[6], _z[3];
    int _corner_of[3];
    ochip_relax_problem *_dev = nullptr;
};

} // namespace

int relax_setup_check(int on)
{
    if (on >= 0)
        g_setup_check.store(on);
    return g_setup_checked.load();
}

bool relax_setup_check_on()
{
    return g_setup_check.load() != 0;
}
void relax_setup_check_passed()
{
    g_setup_checked.fetch_add(1);
}

namespace
{

// runGroundPlane (src/relax/relax.cpp:44-87) as one resident launch on the device (ochip_plane_chain_*, csrc/relax_chain.hip):
// the loop over the poses without an orientation - each takes the orientation of the pose in front of it and is relaxed,
// on its own against the oriented cameras of the graph or together with the group - and the group's own solve behind it.
// Returns 1: the poses up to *resume_pose are done (== nodes.size(): all of them; *all_done: the group's solve too, `surface`
// is written), 0: not taken (something the chain does not do: the caller's loop runs from the first pose), -1: error.
int bootstrap_on_device(ochip_ctx *ctx, const MeasurementGraph &graph, std::vector<NodePose> &nodes,
                        const std::vector<size_t> &edges_to_optimize, surface_model_plane *surface, RelaxTimers *timers,
                        std::string *error, size_t *resume_pose, bool *all_done)
{
    const auto t_begin = clk::now();
    *all_done = false;
    const bool just_this = graph.size_nodes() > 2 * nodes.size(); // relax.cpp:61
    if (std::none_of(nodes.begin(), nodes.end(), [](const NodePose &p) { return hasnan4(p.orientation); }))
        return 0; // every pose has its orientation: nothing to walk
    // cameras: the first pose of every node (the group's solve optimises them all), then the graph's oriented cameras the
    // edges reach.  While one camera is relaxed on its own the others stand as the GRAPH has them (nodeid2poseopt, :182-232):
    // that is what the pose list holds too - RelaxGroup::init copies it - and where it is not, the host loop runs
    camera_table cams(graph, nodes);
    const std::vector<uint32_t> &pose_cam = cams.pose_cam;
    std::vector<size_t> stepped;
    std::vector<char> is_stepped(nodes.size(), 0);
    for (size_t i = 0; i < nodes.size(); i++)
        if (hasnan4(nodes[i].orientation))
        {
            if (pose_cam[i] == UINT32_MAX)
                return 0; // a second pose of a node without an orientation: the host loop knows what that means
            stepped.push_back(i);
            is_stepped[i] = 1;
        }
    std::vector<uint8_t> cam_stepped(cams.n_optimised(), 0); // (a context camera is never stepped)
    for (size_t i = 0; i < nodes.size(); i++)
    {
        if (pose_cam[i] == UINT32_MAX)
            continue;
        cam_stepped[pose_cam[i]] = is_stepped[i] ? 1 : 0;
        if (just_this)
        {
            const MeasurementGraph::Node *n = graph.getNode(nodes[i].node_id);
            if (n == nullptr)
                return 0;
            if (is_stepped[i] ? finite4(n->payload.orientation) && finite3(n->payload.position)
                              : (std::memcmp(n->payload.orientation, nodes[i].orientation, sizeof nodes[i].orientation) != 0 ||
                                 std::memcmp(n->payload.position, nodes[i].position, sizeof nodes[i].position) != 0))
                return 0;
        }
    }
    if (cams.n_optimised() > 330)
        return 0; // (the chain's dense system ends at 1 023 unknowns)
    // the edges in the whitelist's order; gridFilterMatchesPerImage stops at the first one without usable poses
    plane_edge_packer pk;
    const std::vector<ochip_plane_edge> &pe = pk.pe;
    // one camera at a time: a camera without an orientation in the graph is usable only as the step's own camera.  idx1: the
    // first edge with such a camera (u1), idx2: the first edge with another one - or with two of them
    size_t idx1 = SIZE_MAX, idx2 = SIZE_MAX;
    uint32_t u1 = UINT32_MAX;
    for (size_t k = 0; k < edges_to_optimize.size(); k++)
    {
        const MeasurementGraph::Edge *e = graph.getEdge(edges_to_optimize[k]);
        if (e == nullptr)
            continue;
        if (e->source == e->dest)
            return 0;
        const pose_ref a = cams.lookup(e->source), b = cams.lookup(e->dest);
        if (a.loc == nullptr || b.loc == nullptr)
            break; // never usable: nothing gets past it
        const uint32_t ca = a.cam, cb = b.cam;
        if (idx2 == SIZE_MAX)
        {
            const bool sa = ca < cam_stepped.size() && cam_stepped[ca] != 0, sb = cb < cam_stepped.size() && cam_stepped[cb] != 0;
            if (sa && sb)
                idx2 = pe.size(), idx1 = std::min(idx1, idx2);
            else if (sa || sb)
            {
                const uint32_t u = sa ? ca : cb;
                if (idx1 == SIZE_MAX)
                    idx1 = pe.size(), u1 = u;
                else if (u != u1)
                    idx2 = pe.size();
            }
        }
        pk.add(graph, *e, ca, cb);
    }
    const uint64_t n_inliers = pk.n_inliers;
    host_staging inl(ctx);
    if (!inl.alloc((n_inliers ? n_inliers : 1) * sizeof(ochip_plane_inlier), error))
        return -1;
    ochip_plane_inlier *const rec = static_cast<ochip_plane_inlier *>(inl.p);
    pk.pack_inliers(rec);
    // the steps: the poses without an orientation in the list's order, then the group's own solve
    std::vector<ochip_plane_chain_step> steps;
    steps.reserve(stepped.size() + 1);
    steps.resize(stepped.size());
    double tri_all[6], z_all = 0;
    int corner_of[3] = {0, 1, 2};
    {
        std::vector<const double *> positions;
        for (size_t i = 0; i < nodes.size(); i++)
            if (pose_cam[i] != UINT32_MAX)
                positions.push_back(nodes[i].position);
        bootstrap_plane(positions, tri_all, &z_all, corner_of);
    }
    const double down[4] = {std::sin(M_PI / 2), 0.0, 0.0, std::cos(M_PI / 2)}; // DOWN_ORIENTED_NORTH, relax.cpp:12
    for (size_t k = 0; k < stepped.size(); k++)
    {
        const size_t i = stepped[k];
        ochip_plane_chain_step &st = steps[k];
        st.cam = pose_cam[i];
        st.mode = just_this ? 0u : 1u;
        st.prev_cam = -1;
        if (i == 0)
            std::memcpy(st.prev_q, down, sizeof down);
        else
        {
            // previous = the pose in front, as it is when this step starts: a camera of the chain's state where the chain moves
            // it (a stepped camera; with the group every first pose), else what the pose list holds
            const bool moving = pose_cam[i - 1] != UINT32_MAX && (just_this ? is_stepped[i - 1] != 0 : true);
            if (moving)
                st.prev_cam = (int32_t)pose_cam[i - 1];
            std::memcpy(st.prev_q, nodes[i - 1].orientation, sizeof st.prev_q);
        }
        if (just_this)
        {
            bootstrap_plane({nodes[i].position}, st.tri_xy, &st.z0);
            const size_t own = pose_cam[i] == u1 ? idx2 : idx1;
            st.n_filter = (uint32_t)std::min(pe.size(), own);
        }
        else
        {
            std::memcpy(st.tri_xy, tri_all, sizeof tri_all);
            st.z0 = z_all;
            st.n_filter = (uint32_t)pe.size();
        }
    }
    {
        ochip_plane_chain_step st{}; // runGroundPlane's last problem (relax.cpp:81-84)
        st.cam = 0;
        st.mode = 2u;
        st.prev_cam = -1;
        std::memcpy(st.prev_q, down, sizeof down);
        std::memcpy(st.tri_xy, tri_all, sizeof tri_all);
        st.z0 = z_all;
        st.n_filter = (uint32_t)pe.size();
        steps.push_back(st);
    }
    // OCHIP_TEST_HOOKS=chain_partial: the chain takes the first half of the poses only and leaves the rest - and the group's own
    // solve - to the caller's loop, as it does when a step needs the host's grid filter or a wait on the device runs out
    const size_t n_planned = steps.size(); // every pose without an orientation, then the group
    if (ochip_test_hook("chain_partial") && stepped.size() >= 2)
        steps.resize(stepped.size() / 2);
    ochip_plane_chain *chain = nullptr;
    const int crc = ochip_plane_chain_create(ctx, pe.data(), (uint32_t)pe.size(), rec, n_inliers, cams.pos.data(), cams.q.data(),
                                             cams.optimize.data(), (uint32_t)cams.size(), pk.models10.data(), pk.n_models(), 0.15,
                                             1 * M_PI / 180, 1e-3, steps.data(), (uint32_t)steps.size(), &chain);
    if (crc == OCHIP_EINVAL)
        return 0; // (not for the chain: the host loop)
    if (crc != OCHIP_OK)
    {
        device_fail(ctx, error, "ochip_plane_chain_create");
        return -1;
    }
    if (timers)
        timers->setup_host += since(t_begin);
    const auto t_run = clk::now();
    std::vector<double> q_out(cams.q.size());
    ochip_plane_chain_result res{};
    const int rrc = ochip_plane_chain_run(chain, ochip_test_hook("chain_stepped") ? 1 : 0, q_out.data(), &res);
    ochip_plane_chain_destroy(chain);
    if (rrc != OCHIP_OK)
    {
        device_fail(ctx, error, "ochip_plane_chain_run");
        return -1;
    }
    if (ochip_verbose("relax"))
        fprintf(stderr, "[relax chain] %zu poses without an orientation (%s) + the group, %zu edges, %llu inlier matches: %u steps done (status %d), "
                        "%d solves, %d iterations, %d grid syncs on %d workgroups, %.3f ms\n",
                stepped.size(), just_this ? "one at a time" : "with the group", pe.size(), (unsigned long long)n_inliers, res.steps_done, res.status,
                res.solves, res.iterations_total, res.grid_syncs, res.workgroups, since(t_run) * 1e3);
    if (timers)
    {
        timers->device += since(t_run);
        timers->solves += res.solves;
        timers->iterations_total += res.iterations_total;
        timers->last_iterations = res.last_iterations;
        timers->last_initial_cost = res.last_initial_cost;
        timers->last_final_cost = res.last_final_cost;
        timers->last_residual_blocks = res.last_residual_blocks;
    }
    // what relax() wrote back after every finished step
    const bool everything = res.steps_done >= n_planned;
    if (just_this && !everything)
    {
        for (size_t k = 0; k < res.steps_done && k < stepped.size(); k++)
            std::memcpy(nodes[stepped[k]].orientation, &q_out[4 * (size_t)pose_cam[stepped[k]]], 4 * sizeof(double));
    }
    else if (res.steps_done > 0)
        for (size_t i = 0; i < nodes.size(); i++)
            if (pose_cam[i] != UINT32_MAX)
                std::memcpy(nodes[i].orientation, &q_out[4 * (size_t)pose_cam[i]], 4 * sizeof(double));
    *resume_pose = res.steps_done >= stepped.size() ? nodes.size() : stepped[res.steps_done];
    if (everything)
    {
        *all_done = true;
        if (surface)
            for (int i = 0; i < 3; i++)
            {
                surface->corner[corner_of[i]][0] = tri_all[2 * i];
                surface->corner[corner_of[i]][1] = tri_all[2 * i + 1];
                surface->corner[corner_of[i]][2] = res.plane_z[i];
            }
    }
    return 1;
}

} // namespace

bool relax_ground_plane(ochip_ctx *ctx, const MeasurementGraph &graph, std::vector<NodePose> &nodes,
                        const std::vector<size_t> &edges_to_optimize, surface_model_plane *surface,
                        RelaxTimers *timers, std::string *error, const RelaxShard *shard)
{
    // runGroundPlane (src/relax/relax.cpp:44-87)
    auto run = [&](std::vector<NodePose> &poses, surface_model_plane *out) -> bool {
        auto t0 = clk::now();
        GroundPlaneProblem rp(ctx, graph, poses);
        if (!rp.setup(edges_to_optimize, error, shard))
            return false;
        if (timers)
            timers->setup_host += since(t0);
        t0 = clk::now();
        const bool ok = rp.relax_observed_model_only(timers, error) && rp.solve(timers, error);
        if (timers)
            timers->device += since(t0);
        if (ok && out)
            rp.surface(out);
        return ok;
    };
    // DOWN_ORIENTED_NORTH = Quaterniond(AngleAxisd(M_PI, UnitX)), relax.cpp:12
    double previous[4] = {std::sin(M_PI / 2), 0.0, 0.0, std::cos(M_PI / 2)};
    // the poses without an orientation: one resident launch walks them on the device (csrc/relax_chain.hip); what it does not
    // take - and OCHIP_TEST_HOOKS=host_bootstrap - goes through the loop below, a problem and two solves per camera
    size_t first = 0;
    const bool sharded = shard && (shard->world > 1 || shard->exchange);
    if (!sharded && !ochip_test_hook("host_bootstrap"))
    {
        size_t resume = 0;
        bool all_done = false;
        const int brc = bootstrap_on_device(ctx, graph, nodes, edges_to_optimize, surface, timers, error, &resume, &all_done);
        if (brc < 0)
            return false;
        if (all_done)
            return true;
        if (brc > 0)
        {
            first = resume;
            if (first > 0 && first <= nodes.size())
                std::memcpy(previous, nodes[first - 1].orientation, sizeof previous);
        }
    }
    for (size_t i = first; i < nodes.size(); i++)
    {
        NodePose &node = nodes[i];
        if (hasnan4(node.orientation))
        {
            std::memcpy(node.orientation, previous, sizeof previous);
            if (graph.size_nodes() > 2 * nodes.size())
            {
                std::vector<NodePose> justThis{node};
                if (!run(justThis, nullptr))
                    return false;
                node = justThis[0];
            }
            else if (!run(nodes, nullptr))
                return false;
        }
        std::memcpy(previous, node.orientation, sizeof previous);
    }
    return run(nodes, surface);
}

} // namespace opencalibration_amd
