// Points per triangle over the flat locate table (csrc/mesh_locate.hpp): the counter that
// refineByPointDensity and the DENSE_MESH_RELAX state take instead of the host's count_points.  It holds a cloud - on the
// device when it was made with a context (ochip_mesh_points, uploaded once), else in host memory - and counts it against
// any mesh: flat table, locate and per-triangle sums by the device or by the same header in straight loops (locate under
// OpenMP, sums sequentially in point order), then on the host the points whose walk ran out of steps (brute force, added in
// their place in point order), the rows in first-point order, mean and variance.  Both routes give countPointsPerTriangle's
// rows bit for bit.
#pragma once

#include "refine_mesh.hpp"

struct ochip_mesh_points;

namespace opencalibration_amd
{

class MeshPointsCounter : public PointCounter
{
  public:
    // ctx == nullptr: the CPU route.  max_steps: the walk's limit (the public routes pass 100)
    MeshPointsCounter(ochip_ctx *ctx, const std::vector<point_cloud> &clouds, int max_steps = 100);
    MeshPointsCounter(ochip_ctx *ctx, const double *xyz, size_t n, int max_steps = 100);
    ~MeshPointsCounter() override;
    MeshPointsCounter(const MeshPointsCounter &) = delete;
    MeshPointsCounter &operator=(const MeshPointsCounter &) = delete;

    TrianglePointRows count(const MeshGraph &mesh, const std::vector<size_t> &order) override;
    TrianglePointRows count(const MeshGraph &mesh); // edges in id order, as countPointsPerTriangle
    // the triangle of every point (edgeId NONE outside the mesh); false when the device failed
    bool locate(const MeshGraph &mesh, std::vector<TriangleId> *out);
    bool failed() const override
    {
        return !_error.empty();
    }
    const std::string &error() const
    {
        return _error;
    }
    size_t last_exhausted() const // points of the last count whose walk ran out of steps
    {
        return _last_exhausted;
    }

  private:
    struct Raw; // per triangle count / first / sum / sum_sq, per point where (resolved)
    bool run(const MeshGraph &mesh, const std::vector<size_t> *order, FlatLocateTable &tab, Raw &raw, bool want_where);
    void upload();
    ochip_ctx *_ctx;
    int _max_steps;
    std::vector<double> _xyz; // [n][3]
    ochip_mesh_points *_dev = nullptr;
    std::string _error;
    size_t _last_exhausted = 0;
};

} // namespace opencalibration_amd
