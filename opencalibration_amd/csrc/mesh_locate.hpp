// The triangle under a point of a surface mesh, over a flat table: what TriangleLocator::find (host/refine_mesh.cpp; the
// reference's src/surface/refine_mesh.cpp:572-711) does over a MeshGraph, restated over plain arrays so that one text serves
// the CPU route (host/mesh_points.cpp) and the kernel (mesh_points.hip).  DESIGN.md section 4.14.
//
// The table is built on the host by TriangleLocator::flatten.  Per located triangle, in the locator's order: the x, y of its
// three vertices (source, dest, opposite), its three neighbours as triangle indices (0: across its own edge, 1 and 2: across
// the edges dest-opposite and opposite-source as find resolves them; NONE on a border and wherever find gives up), the
// plane of countPointsPerTriangle (origin = the first vertex, unit normal: square root and division stay on the host), and
// the bucket grid over the centroids.  Everything is fp64 and every expression is the host's, in its order; both sides
// build with -ffp-contract=off.
#pragma once

#include <cstddef>
#include <cstdint>

#include <cmath>
#include <string>

#if defined(__HIPCC__)
#define OCHIP_ML_HD __host__ __device__ inline
#else
#define OCHIP_ML_HD inline
#endif

namespace ochip_ml
{

constexpr uint32_t NONE = 0xFFFFFFFFu;      // no triangle: outside the mesh
constexpr uint32_t EXHAUSTED = 0x80000000u; // walk(): max_steps ran out; the low 31 bits are the triangle it stood on
constexpr uint32_t MAX_TRIANGLES = 0x7FFFFFFFu;

struct table
{
    uint32_t T = 0;            // located triangles
    const double *vxy = nullptr;   // [T][6]: x0 y0 x1 y1 x2 y2
    const uint32_t *nbr = nullptr; // [T][3]
    const double *plane = nullptr; // [T][6]: origin x y z, normal x y z
    const double *cx = nullptr, *cy = nullptr; // [T] centroids
    double x0 = 0, y0 = 0, cell = 1;
    int32_t nx = 1;                  // the grid is nx x nx cells
    const uint32_t *start = nullptr; // [nx * nx + 1]
    const uint32_t *items = nullptr; // [T]
};

// The triangle with the nearest centroid (T >= 1): rings of grid cells around the point's cell; on equal distance the lower
// index wins; the search ends with the first ring r whose inner radius r * cell exceeds the best distance, or at `far`.
OCHIP_ML_HD uint32_t nearest_centroid(const table &t, double x, double y)
{
    uint32_t best = 0;
    double bd = INFINITY;
    const long long nx = t.nx;
    const long long cx = (long long)floor((x - t.x0) / t.cell), cy = (long long)floor((y - t.y0) / t.cell);
    auto labs_ = [](long long v) { return v < 0 ? -v : v; };
    auto max_ = [](long long a, long long b) { return a > b ? a : b; };
    auto min_ = [](long long a, long long b) { return a < b ? a : b; };
    const long long far = max_(max_(labs_(cx), labs_(cx - (nx - 1))), max_(labs_(cy), labs_(cy - (nx - 1))));
    auto visit = [&](long long gx, long long gy) {
        if (gx < 0 || gy < 0 || gx >= nx || gy >= nx)
            return;
        const size_t c = (size_t)gy * (size_t)nx + (size_t)gx;
        for (uint32_t it = t.start[c]; it < t.start[c + 1]; it++)
        {
            const uint32_t i = t.items[it];
            const double dx = t.cx[i] - x, dy = t.cy[i] - y, d = dx * dx + dy * dy;
            if (d < bd || (d == bd && i < best))
            {
                bd = d;
                best = i;
            }
        }
    };
    for (long long r = 0; r <= far; r++)
    {
        if (r == 0)
            visit(cx, cy);
        else
        {
            for (long long gx = max_(0, cx - r); gx <= min_(nx - 1, cx + r); gx++)
            {
                visit(gx, cy - r);
                visit(gx, cy + r);
            }
            for (long long gy = max_(0, cy - r + 1); gy <= min_(nx - 1, cy + r - 1); gy++)
            {
                visit(cx - r, gy);
                visit(cx + r, gy);
            }
        }
        if (bd < (double)r * t.cell * (double)r * t.cell)
            break;
    }
    return best;
}

// From `start` across the most violated edge, at most max_steps triangles: the triangle that holds (x, y) - a point on an
// edge or a vertex belongs to the first triangle reached -, NONE where the walk leaves the mesh, or EXHAUSTED | the triangle
// it stood on when the steps ran out (the caller then scans the mesh on the host).
OCHIP_ML_HD uint32_t walk(const table &t, uint32_t start, double x, double y, int max_steps)
{
    uint32_t current = start;
    for (int step = 0; step < max_steps; step++)
    {
        const double *v = t.vxy + (size_t)current * 6;
        auto sign = [](double px, double py, double ax, double ay, double bx, double by) {
            return (px - bx) * (ay - by) - (ax - bx) * (py - by);
        };
        const double d[3] = {sign(x, y, v[0], v[1], v[2], v[3]), sign(x, y, v[2], v[3], v[4], v[5]), sign(x, y, v[4], v[5], v[0], v[1])};
        const bool neg = d[0] < 0 || d[1] < 0 || d[2] < 0, pos = d[0] > 0 || d[1] > 0 || d[2] > 0;
        if (!(neg && pos))
            return current;
        const bool expect_positive = ((d[0] < 0) + (d[1] < 0) + (d[2] < 0)) < 2;
        double worst = 0;
        int leave = -1;
        for (int i = 0; i < 3; i++)
        {
            if (d[i] == 0)
            {
                worst = 0.000001;
                leave = i;
            }
            else if ((d[i] > 0) != expect_positive && fabs(d[i]) > worst)
            {
                worst = fabs(d[i]);
                leave = i;
            }
        }
        if (leave < 0)
            return NONE;
        const uint32_t next = t.nbr[(size_t)current * 3 + leave];
        if (next == NONE)
            return NONE;
        current = next;
    }
    return EXHAUSTED | current;
}

// The signed distance of p to triangle tri's plane, countPointsPerTriangle's expression
OCHIP_ML_HD double plane_distance(const table &t, uint32_t tri, double px, double py, double pz)
{
    const double *o = t.plane + (size_t)tri * 6, *n = o + 3;
    return (px - o[0]) * n[0] + (py - o[1]) * n[1] + (pz - o[2]) * n[2];
}

// What a table must satisfy before nearest_centroid / walk may read it (n_start, n_items: the lengths of start and items
// as the caller holds them).  Empty string: consistent; else what is wrong.  A table with T = 0 holds nothing to read.
inline std::string validate(const table &t, size_t n_start, size_t n_items)
{
    if (t.T == 0)
        return "";
    if (t.T > MAX_TRIANGLES)
        return "more than 2^31 - 1 triangles";
    if (!t.vxy || !t.nbr || !t.plane || !t.cx || !t.cy || !t.start || !t.items)
        return "an array of the table is NULL";
    if (t.nx < 1 || t.nx > 1024)
        return "the grid side " + std::to_string(t.nx) + " is outside 1 .. 1024";
    if (!(t.cell > 0) || !std::isfinite(t.cell) || !std::isfinite(t.x0) || !std::isfinite(t.y0))
        return "the grid's origin or cell size is not a finite positive number";
    const size_t cells = (size_t)t.nx * (size_t)t.nx;
    if (n_start != cells + 1)
        return "start has " + std::to_string(n_start) + " entries, the grid needs " + std::to_string(cells + 1);
    if (n_items != t.T)
        return "items has " + std::to_string(n_items) + " entries for " + std::to_string(t.T) + " triangles";
    if (t.start[0] != 0)
        return "start[0] is not 0";
    for (size_t c = 0; c < cells; c++)
        if (t.start[c + 1] < t.start[c])
            return "start is not monotone at cell " + std::to_string(c);
    if (t.start[cells] != t.T)
        return "start ends at " + std::to_string(t.start[cells]) + ", not at the number of triangles";
    for (size_t i = 0; i < n_items; i++)
        if (t.items[i] >= t.T)
            return "item " + std::to_string(i) + " names triangle " + std::to_string(t.items[i]) + " of " + std::to_string(t.T);
    for (size_t i = 0; i < (size_t)t.T * 3; i++)
        if (t.nbr[i] != NONE && t.nbr[i] >= t.T)
            return "neighbour " + std::to_string(i % 3) + " of triangle " + std::to_string(i / 3) + " is " + std::to_string(t.nbr[i]) +
                   " of " + std::to_string(t.T);
    return "";
}

} // namespace ochip_ml
