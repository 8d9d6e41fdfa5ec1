// Height of the mesh under an orthomosaic / DSM pixel, shared by the device kernels (ortho.hip, hipcc) and the host's
// CPU route (host/ortho.cpp, g++), both built with -ffp-contract=off so that the two agree to the bit.
//
// The ray is the reference's vertical one, {dir (0, 0, -1), origin (x, y, mean_camera_z)} (src/ortho/ortho.cpp:553-554,
// 823-824).  The walker's predicates (src/surface/intersect.cpp:71-105, geometry/utils.hpp:10-14): a triangle is first put
// in the order the walker keeps (corners 0 and 1 swapped when crossZ(c0, c1, c2) < 0), the plane is
// cornerPlane2normOffsetPlane (offset corner 0, normal (c0 - c1) x (c0 - c2) normalised as Eigen does) and the hit is
// rayPlaneIntersection (|n . dir| < 1e-9: parallel); the hit is outside when some edge gives crossZ(hit, ci, ci+1) < 0,
// so a point exactly on an edge is inside.
//
// The corners come in the project's canonical order (ascending mesh node index): the walker's own order depends on the
// path it walked, and so do the last bits of its z.  Both routes evaluate the triangle they found in this one order.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define OCHIP_OG __host__ __device__ inline
#else
#define OCHIP_OG inline
#endif

namespace ochip_og
{

OCHIP_OG bool cross_z_negative(double ax, double ay, double bx, double by, double cx, double cy)
{
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) < 0;
}

// c9: three corners xyz.  Returns true with *z set when the vertical ray through (x, y) meets the triangle's plane inside
// the triangle; false when the point is outside or the plane is parallel to the ray (or the hit is NaN).  test_inside =
// false: the plane's height whatever the point (a walk that ran out of steps reports the triangle it stands on).
OCHIP_OG bool triangle_height(const double *c9, double x, double y, double mean_camera_z, double *z, bool test_inside = true)
{
    double c[3][3] = {{c9[0], c9[1], c9[2]}, {c9[3], c9[4], c9[5]}, {c9[6], c9[7], c9[8]}};
    if (cross_z_negative(c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1]))
        for (int k = 0; k < 3; k++)
        {
            const double t = c[0][k];
            c[0][k] = c[1][k];
            c[1][k] = t;
        }
    // inside test first (the walker tests the hit, whose x / y are x + 0 * t, y + 0 * t: x and y whenever t is finite,
    // and a non-finite t is rejected below)
    for (int i = 0; i < 3 && test_inside; i++)
        if (cross_z_negative(x, y, c[i][0], c[i][1], c[(i + 1) % 3][0], c[(i + 1) % 3][1]))
            return false;
    const double ux = c[0][0] - c[1][0], uy = c[0][1] - c[1][1], uz = c[0][2] - c[1][2];
    const double vx = c[0][0] - c[2][0], vy = c[0][1] - c[2][1], vz = c[0][2] - c[2][2];
    double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double n2 = nx * nx + ny * ny + nz * nz;
    if (n2 > 0)
    {
        const double nn = sqrt(n2);
        nx = nx / nn;
        ny = ny / nn;
        nz = nz / nn;
    }
    const double denom = nx * 0.0 + ny * 0.0 + nz * -1.0;
    if (fabs(denom) < 1e-9)
        return false;
    const double t = ((nx * c[0][0] + ny * c[0][1] + nz * c[0][2]) - (x * nx + y * ny + mean_camera_z * nz)) / denom;
    const double hx = x + 0.0 * t, hy = y + 0.0 * t, hz = mean_camera_z + -1.0 * t;
    if (hx != hx || hy != hy || hz != hz)
        return false;
    *z = hz;
    return true;
}

// The uniform bin grid over one surface's triangles: cell of coordinate v along an axis with origin o, edge `cell`
// and n cells; -1 below the origin.  Monotonic in v, so a triangle binned by its bounding box's corners is found from
// every point of the box.
OCHIP_OG int grid_cell(double v, double o, double cell, int n)
{
    const double f = (v - o) / cell;
    if (!(f >= 0))
        return -1;
    return f < (double)n ? (int)f : n - 1;
}

// the camera ray of image_from_3d(point, model, position, orientation_inverse) (include/opencalibration/distort/
// distort_keypoints.hpp:79-86): R_inv * (p - position) in Eigen's coefficient order.  cam: the 24-double record of
// ochip_ortho_thumbnail (position 3, R_inv 9 row-major, f, ppx, ppy, k1, k2, k3, p1, p2, thumb_scale, rows, cols, 0).
// The projection itself is the device's dense-style restatement in ortho.hip and the host's image_from_3d
// (host/invert_distortion.cpp) on the CPU route: two independent codes, held to the bit by the tests.
OCHIP_OG double camera_ray_z(const double *cam, double px, double py, double pz, double ray[3])
{
    const double d[3] = {px - cam[0], py - cam[1], pz - cam[2]};
    const double *R = cam + 3;
    for (int i = 0; i < 3; i++)
        ray[i] = R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2];
    return ray[2];
}

// searchKnn({x, y}, 5) as a running list: squared XY distance, then camera order (cameras offered in ascending order,
// so a strict < keeps the earlier of two equal distances first)
constexpr int KNN = 5;
OCHIP_OG void knn_offer(double d, uint32_t id, double bd[KNN], uint32_t bi[KNN])
{
    if (!(d < bd[KNN - 1]))
        return;
    for (int k = 0; k < KNN; k++)
        if (d < bd[k])
        {
            const double td = bd[k];
            const uint32_t ti = bi[k];
            bd[k] = d, bi[k] = id;
            d = td, id = ti;
        }
}

// a kNN list before the first offer: no distance, every entry `none` (the caller's "no camera" sentinel)
OCHIP_OG void knn_init(uint32_t none, double bd[KNN], uint32_t bi[KNN])
{
    for (int k = 0; k < KNN; k++)
        bd[k] = INFINITY, bi[k] = none;
}

// The brute-force search every pruned one is held to: the list of (x, y) over cameras 0 .. n - 1 of a table of `stride`
// doubles per record (x, y first), offered in ascending order.  Fewer than 5 cameras leave `none` entries at the end.
OCHIP_OG void knn_brute(const double *cams, size_t stride, size_t n, double x, double y, uint32_t none, double bd[KNN],
                        uint32_t bi[KNN])
{
    knn_init(none, bd, bi);
    for (size_t i = 0; i < n; i++)
    {
        const double dx = x - cams[i * stride], dy = y - cams[i * stride + 1];
        knn_offer(dx * dx + dy * dy, (uint32_t)i, bd, bi);
    }
}

// ortho.cpp:601-611 for one camera's projection `pixel` (cam: the 24-double record): times thumb_scale, truncated, strictly
// inside the thumbnail.  (int)v > 0 && (int)v < n is v >= 1 && v < n, which also rejects NaN and needs no out-of-range
// conversion.
OCHIP_OG bool thumbnail_cell(const double *cam, const double pixel[2], int *col, int *row)
{
    const double tx = pixel[0] * cam[20], ty = pixel[1] * cam[20];
    if (!(tx >= 1 && tx < cam[22] && ty >= 1 && ty < cam[21]))
        return false;
    *col = (int)tx;
    *row = (int)ty;
    return true;
}

} // namespace ochip_og
