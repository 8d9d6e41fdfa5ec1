// The per-pixel rules of the layered full-resolution orthomosaic (reference: processLayeredTile, src/ortho/ortho.cpp:
// 1206-1429, and its helpers :43-220, src/ortho/blending.cpp:12-36), shared by the device kernels (ortho_layers.hip,
// hipcc) and the host's CPU route (host/ortho_layers.cpp, g++).  Both are built with -ffp-contract=off and use only
// correctly rounded operations here (+ - * /, sqrt, ceil, rint, integer ops and tables built on the host), so that the
// two routes agree to the bit.  The kNN that picks the cameras is the only part each route does its own way.
//
// Departure L1: the reference converts colours with cv::cvtColor, whose 8-bit fixed-point tables are not
// restated.  This header implements OpenCV's documented conversion instead: the sRGB transfer curve, the documented
// RGB -> XYZ matrix with the D65 white (Xn 0.950456, Zn 1.088754), CIE L*a*b* with its 0.008856 / 7.787 / 903.3 branch,
// and the 8-bit scaling L * 255 / 100, a + 128, b + 128 rounded to nearest (ties to even) and saturated.  The transfer
// curve's powers are taken on the host only: decoding is a 256-entry table, encoding a search over the 255 thresholds
// that separate two codes; cube roots are a fixed Newton iteration.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define OCHIP_OL __host__ __device__ inline
#else
#define OCHIP_OL inline
#endif

namespace ochip_ol
{

// ---- L1: colour conversion ------------------------------------------------------------------------------------------

struct lab_tables
{
    double lin[256]; // the sRGB transfer curve of code v / 255, linear
    double thr[255]; // thr[k]: the linear value half way (in code space) between codes k and k + 1
};

// host only (std::pow): the tables of lab_tables
inline double srgb_decode(double c)
{
    return c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
}
inline void lab_tables_build(lab_tables *t)
{
    for (int v = 0; v < 256; v++)
        t->lin[v] = srgb_decode(v / 255.0);
    for (int k = 0; k < 255; k++)
        t->thr[k] = srgb_decode((k + 0.5) / 255.0);
}

// t^(1/3) for t in (0.008856, 2): Newton's iteration from above (1 or t), a fixed 16 steps
OCHIP_OL double cbrt_newton(double t)
{
    double y = t > 1.0 ? t : 1.0;
    for (int i = 0; i < 16; i++)
        y = (2.0 * y + t / (y * y)) / 3.0;
    return y;
}

OCHIP_OL double lab_f(double t)
{
    return t > 0.008856 ? cbrt_newton(t) : 7.787 * t + 16.0 / 116.0;
}

// BGR codes -> L*a*b* (L in 0..100)
OCHIP_OL void lab_from_bgr(const lab_tables &T, const uint8_t bgr[3], double lab[3])
{
    const double B = T.lin[bgr[0]], G = T.lin[bgr[1]], R = T.lin[bgr[2]];
    // Each row of the matrix sums to its white (0.412453 + 0.357580 + 0.180423 = 0.950456, .. = 1, .. = 1.088754), so
    // X / Xn, Y and Z / Zn are G plus multiples of R - G and B - G: a grey (R = G = B) has the three equal to the bit, and
    // a = b = 0 exactly, where the plain row sums left them at 1e-13.
    const double dR = R - G, dB = B - G;
    const double X = G + (0.412453 / 0.950456) * dR + (0.180423 / 0.950456) * dB;
    const double Y = G + 0.212671 * dR + 0.072169 * dB;
    const double Z = G + (0.019334 / 1.088754) * dR + (0.950227 / 1.088754) * dB;
    const double fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    lab[0] = Y > 0.008856 ? 116.0 * fy - 16.0 : 903.3 * Y;
    lab[1] = 500.0 * (fx - fy);
    lab[2] = 200.0 * (fy - fz);
}

OCHIP_OL uint8_t sat8(double v)
{
    const double r = rint(v);
    return r <= 0 ? 0 : r >= 255 ? 255 : (uint8_t)r; // NaN -> 255 (cannot occur: every input is finite)
}

// cv::COLOR_BGR2Lab on CV_8UC3, restated (L1)
OCHIP_OL void lab8_from_bgr8(const lab_tables &T, const uint8_t bgr[3], uint8_t lab8[3])
{
    double lab[3];
    lab_from_bgr(T, bgr, lab);
    lab8[0] = sat8(lab[0] * 255.0 / 100.0);
    lab8[1] = sat8(lab[1] + 128.0);
    lab8[2] = sat8(lab[2] + 128.0);
}

// cv::COLOR_BGR2Lab on the CV_32FC3 image convertTo(.., 1 / 255) makes of 8-bit codes, restated (L1)
OCHIP_OL void labf_from_bgr8(const lab_tables &T, const uint8_t bgr[3], float labf[3])
{
    double lab[3];
    lab_from_bgr(T, bgr, lab);
    labf[0] = (float)lab[0], labf[1] = (float)lab[1], labf[2] = (float)lab[2];
}

// linear -> the nearest sRGB code in code space: the number of thresholds at or below v
OCHIP_OL uint8_t srgb_encode8(const lab_tables &T, double v)
{
    int lo = 0, hi = 255; // answer in [lo, hi]
    while (lo < hi)
    {
        const int mid = (lo + hi) / 2; // code > mid iff v >= thr[mid]
        if (v >= T.thr[mid])
            lo = mid + 1;
        else
            hi = mid;
    }
    return (uint8_t)lo;
}

OCHIP_OL double lab_f_inv(double f)
{
    return f > 0.206893 ? f * f * f : (f - 16.0 / 116.0) / 7.787;
}

// cv::COLOR_Lab2BGR on CV_8UC3, restated (L1): the documented XYZ -> RGB matrix
OCHIP_OL void bgr8_from_lab8(const lab_tables &T, const uint8_t lab8[3], uint8_t bgr[3])
{
    const double L = lab8[0] * 100.0 / 255.0, a = lab8[1] - 128.0, b = lab8[2] - 128.0;
    double Y, fy;
    if (L <= 8.0)
    {
        Y = L / 903.3;
        fy = 7.787 * Y + 16.0 / 116.0;
    }
    else
    {
        fy = (L + 16.0) / 116.0;
        Y = fy * fy * fy;
    }
    const double X = lab_f_inv(fy + a / 500.0) * 0.950456;
    const double Z = lab_f_inv(fy - b / 200.0) * 1.088754;
    const double R = 3.240479 * X - 1.53715 * Y - 0.498535 * Z;
    const double G = -0.969256 * X + 1.875991 * Y + 0.041556 * Z;
    const double B = 0.055648 * X - 0.204043 * Y + 1.057311 * Z;
    bgr[0] = srgb_encode8(T, B);
    bgr[1] = srgb_encode8(T, G);
    bgr[2] = srgb_encode8(T, R);
}

// ---- the sample's bookkeeping ---------------------------------------------------------------------------------------

// acos(x) for x in [-1, 1] from + - * / sqrt: asin's series on |y| <= 0.5 (40 terms, each at most 0.25^n of the first)
OCHIP_OL double asin_series(double y)
{
    const double y2 = y * y;
    double term = y, sum = y;
    for (int n = 0; n < 40; n++)
    {
        term = term * y2 * (double)((2 * n + 1) * (2 * n + 1)) / (double)((2 * n + 2) * (2 * n + 3));
        sum = sum + term;
    }
    return sum;
}
OCHIP_OL double acos_restated(double x)
{
    const double pi = 3.141592653589793;
    if (x > 0.5)
        return 2.0 * asin_series(sqrt((1.0 - x) / 2.0));
    if (x < -0.5)
        return pi - 2.0 * asin_series(sqrt((1.0 + x) / 2.0));
    return pi / 2.0 - asin_series(x);
}

// normalizedImageRadius (ortho.cpp:43-57)
OCHIP_OL float normalized_radius(double px, double py, int width, int height)
{
    if (width <= 0 || height <= 0)
        return 0.0f;
    const double half_w = width * 0.5, half_h = height * 0.5;
    const double dx = (px - half_w) / half_w, dy = (py - half_h) / half_h;
    double r = sqrt(dx * dx + dy * dy) * 0.7071067811865475;
    r = r < 0.0 ? 0.0 : r > 1.0 ? 1.0 : r;
    return (float)r;
}

// normalizedImagePosition (ortho.cpp:59-67)
OCHIP_OL void normalized_position(double px, double py, int width, int height, float *nx, float *ny)
{
    if (width <= 0 || height <= 0)
    {
        *nx = *ny = 0.0f;
        return;
    }
    const float x = (float)((px - width * 0.5) / (width * 0.5));
    const float y = (float)((py - height * 0.5) / (height * 0.5));
    *nx = x < -1.0f ? -1.0f : x > 1.0f ? 1.0f : x;
    *ny = y < -1.0f ? -1.0f : y > 1.0f ? 1.0f : y;
}

OCHIP_OL float minf(float a, float b)
{
    return b < a ? b : a; // std::min
}

// computeBlendWeight (src/ortho/blending.cpp:12-36), float throughout
OCHIP_OL float blend_weight(float px, float py, int width, int height, float camera_distance)
{
    const float half_w = width * 0.5f, half_h = height * 0.5f;
    const float min_edge = minf(minf(minf(px, width - 1.0f - px), py), height - 1.0f - py);
    float edge = minf(min_edge / half_w, 1.0f);
    edge = edge < 0.001f ? 0.001f : edge;
    const float cx = (px - half_w) / half_w, cy = (py - half_h) / half_h;
    const float center_dist = sqrtf(cx * cx + cy * cy);
    const float center = 1.0f - 0.5f * minf(center_dist, 1.0f);
    const float proximity = 1.0f / (1.0f + camera_distance * camera_distance);
    return edge * center * proximity;
}

// ---- projection and its Jacobian ------------------------------------------------------------------------------------

// a value and its partials in world x and y (ceres::Jet<double, 2>'s arithmetic)
struct jet
{
    double a, v0, v1;
};
OCHIP_OL jet jc(double a)
{
    return jet{a, 0.0, 0.0};
}
OCHIP_OL jet operator+(jet x, jet y)
{
    return jet{x.a + y.a, x.v0 + y.v0, x.v1 + y.v1};
}
OCHIP_OL jet operator-(jet x, jet y)
{
    return jet{x.a - y.a, x.v0 - y.v0, x.v1 - y.v1};
}
OCHIP_OL jet operator*(jet x, jet y)
{
    return jet{x.a * y.a, x.a * y.v0 + x.v0 * y.a, x.a * y.v1 + x.v1 * y.a};
}
OCHIP_OL jet operator*(double s, jet x)
{
    return jet{s * x.a, s * x.v0, s * x.v1};
}
OCHIP_OL jet operator/(jet x, jet y)
{
    const double inv = 1.0 / y.a, q = x.a * inv;
    return jet{q, (x.v0 - q * y.v0) * inv, (x.v1 - q * y.v1) * inv};
}

// The camera record of the layered render, CAM_DOUBLES doubles: position 3, R_inv 9 (row-major; orientation.inverse()
// .toRotationMatrix()), f, ppx, ppy, k1, k2, k3, p1, p2, pixels_cols, pixels_rows, camera_down 3 (orientation.inverse() *
// (0, 0, 1)), 3 unused.
constexpr int CAM_DOUBLES = 28;

// image_from_3d(point, model, position, R_inv) (distort_keypoints.hpp:26-86, PLANAR) on jets seeded in x and y: the
// pixel and J = d pixel / d (x, y), row-major.  Returns R_inv (p - position)'s z.
OCHIP_OL double project_jacobian(const double *cam, double x, double y, double z, double pixel[2], double J[4])
{
    const jet d[3] = {jet{x, 1.0, 0.0} - jc(cam[0]), jet{y, 0.0, 1.0} - jc(cam[1]), jc(z) - jc(cam[2])};
    const double *R = cam + 3;
    jet ray[3];
    for (int i = 0; i < 3; i++)
        ray[i] = R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2];
    const jet zc = ray[2].a < 1e-3 ? jc(1e-3) : ray[2];
    const jet p[2] = {ray[0] / zc, ray[1] / zc};
    const double *m = cam + 12; // f ppx ppy k1 k2 k3 p1 p2
    jet r2[3];
    r2[0] = p[0] * p[0] + p[1] * p[1];
    r2[1] = r2[0] * r2[0];
    r2[2] = r2[1] * r2[0];
    const jet radial = m[3] * r2[0] + m[4] * r2[1] + m[5] * r2[2];
    const jet prod = p[0] * p[1];
    for (int i = 0; i < 2; i++)
    {
        const jet dd = (jc(1.0) + radial) * p[i] + m[6 + i] * (2.0 * prod) + m[7 - i] * (r2[0] + 2.0 * p[i] * p[i]);
        const jet px = m[0] * dd + jc(m[1 + i]);
        pixel[i] = px.a;
        J[2 * i] = px.v0;
        J[2 * i + 1] = px.v1;
    }
    return ray[2].a;
}

// ---- PatchSampler::sampleWithJacobian (ortho.cpp:117-213) ----------------------------------------------------------

constexpr int MAX_PATCH_RADIUS = 16;

// img: rows x cols x 3 BGR.  M = (gsd^2 J) J^T, its eigenvalues in closed form (M's lower triangle, as Eigen's
// self-adjoint solver reads it), the ellipse d^T M^-1 d <= 1 with Eigen's 2 x 2 inverse, the members' 8-bit Lab summed in
// double, truncated, back to BGR.  pixel must lie in [0, cols) x [0, rows) (the caller's test).
OCHIP_OL bool patch_sample(const lab_tables &T, const uint8_t *img, int rows, int cols, const double pixel[2],
                           const double J[4], double gsd, uint8_t out[3])
{
    const double s = gsd * gsd;
    const double A[4] = {s * J[0], s * J[1], s * J[2], s * J[3]};
    const double M00 = A[0] * J[0] + A[1] * J[1], M01 = A[0] * J[2] + A[1] * J[3];
    const double M10 = A[2] * J[0] + A[3] * J[1], M11 = A[2] * J[2] + A[3] * J[3];
    const double mean = (M00 + M11) / 2.0, h = (M00 - M11) / 2.0;
    const double disc = sqrt(h * h + M10 * M10);
    const double hi = mean + disc, lo = mean - disc;
    const double a = sqrt(hi > 1e-6 ? hi : 1e-6), b = sqrt(lo > 1e-6 ? lo : 1e-6);
    const int ix = (int)pixel[0], iy = (int)pixel[1];
    const uint8_t *centre = img + ((size_t)iy * (size_t)cols + (size_t)ix) * 3;
    if ((a < 1.0 && b < 1.0) || M00 * M11 - M10 * M01 < 1e-12)
    {
        out[0] = centre[0], out[1] = centre[1], out[2] = centre[2];
        return true;
    }
    // a >= 1 here (ceil of a NaN never reaches the int conversion: a NaN a and b take the branch above)
    const double ra = ceil(a);
    const int radius = ra < MAX_PATCH_RADIUS ? (int)ra : MAX_PATCH_RADIUS;
    const int x0 = ix - radius > 0 ? ix - radius : 0, y0 = iy - radius > 0 ? iy - radius : 0;
    const int x1 = ix + radius < cols - 1 ? ix + radius : cols - 1, y1 = iy + radius < rows - 1 ? iy + radius : rows - 1;
    const double det = M00 * M11 - M10 * M01;
    const double inv = 1.0 / det;
    const double I00 = M11 * inv, I10 = -M10 * inv, I01 = -M01 * inv, I11 = M00 * inv;
    double sum[3] = {0, 0, 0};
    int count = 0;
    for (int py = y0; py <= y1; py++)
        for (int px = x0; px <= x1; px++)
        {
            const double dx = px - pixel[0], dy = py - pixel[1];
            const double e = (dx * I00 + dy * I10) * dx + (dx * I01 + dy * I11) * dy;
            if (!(e <= 1.0))
                continue;
            uint8_t lab[3];
            lab8_from_bgr8(T, img + ((size_t)py * (size_t)cols + (size_t)px) * 3, lab);
            sum[0] += lab[0], sum[1] += lab[1], sum[2] += lab[2];
            count++;
        }
    if (count == 0)
    {
        out[0] = centre[0], out[1] = centre[1], out[2] = centre[2];
        return true;
    }
    const uint8_t mean8[3] = {(uint8_t)(sum[0] / count), (uint8_t)(sum[1] / count), (uint8_t)(sum[2] / count)};
    bgr8_from_lab8(T, mean8, out);
    return true;
}

// ---- one pixel's layers (ortho.cpp:1239-1322) -----------------------------------------------------------------------

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int KNN = 5;
constexpr int MAX_LAYERS = 8;

struct cameras_view
{
    const double *cams;            // [n][CAM_DOUBLES]
    const uint8_t *const *images;  // [n] BGR, pixels_rows x pixels_cols x 3
    uint32_t n;
};

// The band's layer planes, [L][px] each (px = rows * cols of the band): nvalid [px]; cam the camera index (NONE:
// invalid); bgra; id (node id, 0: invalid); weight; fields [L][px][4] = normalized_radius, normalized_x, normalized_y,
// view_angle for the correspondences.
struct band_planes
{
    int L;
    int32_t cols;
    int64_t rows;
    uint8_t *nvalid;
    uint32_t *cam;
    uint8_t *bgra;
    uint64_t *id;
    float *weight; // may be NULL
    float *fields;
};

// Pixel i of the band at world (x, y), height zf (the DSM's float); knn: the 5 nearest cameras (NONE-padded).
OCHIP_OL void pixel_layers(const lab_tables &T, const cameras_view &C, const uint64_t *node_ids, const uint32_t knn[KNN],
                           double x, double y, float zf, double gsd, const band_planes &B, size_t i)
{
    const size_t px = (size_t)B.rows * (size_t)B.cols;
    int n = 0;
    if (zf == zf)
    {
        const double z = zf;
        for (int k = 0; k < KNN && n < B.L; k++)
        {
            if (knn[k] == NONE)
                break;
            const double *c = C.cams + (size_t)knn[k] * CAM_DOUBLES;
            double pixel[2], J[4];
            if (project_jacobian(c, x, y, z, pixel, J) <= 0)
                continue;
            const int cols = (int)c[20], rows = (int)c[21];
            if (!(pixel[0] >= 0 && pixel[0] < cols && pixel[1] >= 0 && pixel[1] < rows))
                continue;
            uint8_t bgr[3];
            if (!patch_sample(T, C.images[knn[k]], rows, cols, pixel, J, gsd, bgr))
                continue;
            const size_t o = (size_t)n * px + i;
            B.cam[o] = knn[k];
            B.id[o] = node_ids[knn[k]];
            uint8_t *q = B.bgra + 4 * o;
            q[0] = bgr[0], q[1] = bgr[1], q[2] = bgr[2], q[3] = 255;
            float *f = B.fields + 4 * o;
            f[0] = normalized_radius(pixel[0], pixel[1], cols, rows);
            normalized_position(pixel[0], pixel[1], cols, rows, &f[1], &f[2]);
            const double t[3] = {x - c[0], y - c[1], z - c[2]};
            const double norm = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            double cosang = norm > 0 ? c[22] * (t[0] / norm) + c[23] * (t[1] / norm) + c[24] * (t[2] / norm)
                                     : c[22] * t[0] + c[23] * t[1] + c[24] * t[2];
            cosang = cosang < -1.0 ? -1.0 : cosang > 1.0 ? 1.0 : cosang;
            f[3] = (float)acos_restated(cosang);
            if (B.weight)
                B.weight[o] = blend_weight((float)pixel[0], (float)pixel[1], cols, rows, (float)norm);
            n++;
        }
    }
    B.nvalid[i] = (uint8_t)n;
    for (int k = n; k < B.L; k++) // the GeoTIFF writer's invalid sample (ortho.cpp:1085-1101)
    {
        const size_t o = (size_t)k * px + i;
        B.cam[o] = NONE;
        B.id[o] = 0;
        B.bgra[4 * o] = B.bgra[4 * o + 1] = B.bgra[4 * o + 2] = B.bgra[4 * o + 3] = 0;
        float *f = B.fields + 4 * o;
        f[0] = f[1] = f[2] = f[3] = 0;
        if (B.weight)
            B.weight[o] = 0;
    }
}

// ---- the colour correspondences (ortho.cpp:1324-1417) of the finished band ------------------------------------------

// the record of ochip.h's ochip_color_corr
struct corr_record
{
    float lab_a[3], lab_b[3];
    uint64_t camera_id_a, camera_id_b;
    uint32_t model_id_a, model_id_b;
    float normalized_radius_a, normalized_radius_b, view_angle_a, view_angle_b;
    float normalized_x_a, normalized_y_a, normalized_x_b, normalized_y_b;
    int32_t row, col;
    uint32_t layer_a, layer_b;
};

struct corr_config
{
    int tile_size, radius, subsample;
    int64_t row0; // the band's first raster row (a multiple of tile_size)
};

// the tile of band-local pixel (r, c): origin and size
OCHIP_OL void tile_of(const band_planes &B, int T, int64_t r, int32_t c, int64_t *r0, int32_t *c0, int64_t *th, int32_t *tw)
{
    *r0 = r / T * T;
    *c0 = c / T * T;
    *th = B.rows - *r0 < T ? B.rows - *r0 : T;
    *tw = B.cols - *c0 < T ? B.cols - *c0 : T;
}

// how many records pixel (r, c) emits: C(n, 2) when it is sampled, else 0
OCHIP_OL int corr_count(const band_planes &B, const corr_config &K, int64_t r, int32_t c)
{
    const size_t i = (size_t)r * (size_t)B.cols + (size_t)c;
    const int n = B.nvalid[i];
    if (n == 0 || K.subsample <= 0)
        return 0;
    int64_t r0, th;
    int32_t c0, tw;
    tile_of(B, K.tile_size, r, c, &r0, &c0, &th, &tw);
    const int64_t lr = r - r0;
    const int32_t lc = c - c0;
    const uint32_t me = B.cam[i];
    bool boundary = false;
    const int dr[4] = {0, 0, -1, 1}, dc[4] = {-1, 1, 0, 0};
    for (int d = 0; d < 4 && !boundary; d++)
    {
        const int64_t nr = lr + dr[d];
        const int32_t nc = lc + dc[d];
        if (nr >= 0 && nr < th && nc >= 0 && nc < tw)
        {
            const size_t j = (size_t)(r0 + nr) * (size_t)B.cols + (size_t)(c0 + nc);
            if (B.nvalid[j] > 0 && B.cam[j] != me)
                boundary = true;
        }
    }
    const bool sampled = boundary ? (lr + lc) % K.subsample == 0 : lr % K.subsample == 0 && lc % K.subsample == 0;
    return sampled ? n * (n - 1) / 2 : 0;
}

// the records of a sampled pixel, (a, b) lexicographically, into out[0 .. C(n, 2))
OCHIP_OL void corr_write(const lab_tables &T, const band_planes &B, const corr_config &K, const uint32_t *model_ids, int64_t r,
                         int32_t c, corr_record *out)
{
    const size_t px = (size_t)B.rows * (size_t)B.cols;
    const size_t i = (size_t)r * (size_t)B.cols + (size_t)c;
    const int n = B.nvalid[i];
    int64_t r0, th;
    int32_t c0, tw;
    tile_of(B, K.tile_size, r, c, &r0, &c0, &th, &tw);
    int w = 0;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++)
        {
            const uint32_t ca = B.cam[(size_t)a * px + i], cb = B.cam[(size_t)b * px + i];
            float sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
            int count = 0;
            for (int dr = -K.radius; dr <= K.radius; dr++)
                for (int dc = -K.radius; dc <= K.radius; dc++)
                {
                    const int64_t kr = r - r0 + dr;
                    const int64_t kc = (int64_t)(c - c0) + dc;
                    if (kr < 0 || kr >= th || kc < 0 || kc >= tw)
                        continue;
                    const size_t j = (size_t)(r0 + kr) * (size_t)B.cols + (size_t)(c0 + kc);
                    // valid in both layers (nvalid > b) and the same cameras as the centre
                    if (B.nvalid[j] <= b || B.cam[(size_t)a * px + j] != ca || B.cam[(size_t)b * px + j] != cb)
                        continue;
                    float la[3], lb[3];
                    labf_from_bgr8(T, B.bgra + 4 * ((size_t)a * px + j), la);
                    labf_from_bgr8(T, B.bgra + 4 * ((size_t)b * px + j), lb);
                    for (int q = 0; q < 3; q++)
                        sa[q] = sa[q] + la[q], sb[q] = sb[q] + lb[q];
                    count++;
                }
            corr_record &o = out[w++];
            const float inv = 1.0f / (float)count; // cv::Vec3f / float scales by the reciprocal; count >= 1 (the centre)
            for (int q = 0; q < 3; q++)
                o.lab_a[q] = sa[q] * inv, o.lab_b[q] = sb[q] * inv;
            const float *fa = B.fields + 4 * ((size_t)a * px + i), *fb = B.fields + 4 * ((size_t)b * px + i);
            o.camera_id_a = B.id[(size_t)a * px + i];
            o.camera_id_b = B.id[(size_t)b * px + i];
            o.model_id_a = model_ids[ca];
            o.model_id_b = model_ids[cb];
            o.normalized_radius_a = fa[0], o.normalized_radius_b = fb[0];
            o.view_angle_a = fa[3], o.view_angle_b = fb[3];
            o.normalized_x_a = fa[1], o.normalized_y_a = fa[2];
            o.normalized_x_b = fb[1], o.normalized_y_b = fb[2];
            o.row = (int32_t)(K.row0 + r);
            o.col = c;
            o.layer_a = (uint32_t)a, o.layer_b = (uint32_t)b;
        }
}

} // namespace ochip_ol
