// The per-pixel and per-level rules of the blended full-resolution orthomosaic (reference: blendLayeredGeoTIFF,
// src/ortho/ortho.cpp:1665-1990, and laplacianBlend / fillInvalidRegions, src/ortho/blending.cpp), shared by the device
// kernels (ortho_blend.hip, hipcc) and the host's CPU route (host/ortho_blend.cpp, g++).  Both are built with
// -ffp-contract=off and use only correctly rounded operations here (+ - * /, sqrt, rint, ldexp, integer ops and the
// host-built tables of ortho_layers.hpp), so that the two routes agree to the bit.  Only the chamfer distance is computed
// each route its own way (a sequential two-pass here, a row scan on the device); it is exact in integers, so both agree.
//
// The defined behaviours (beside L1):
//   pyrDown / pyrUp: the documented 5 x 5 kernel [1 4 6 4 1]^T [1 4 6 4 1] / 256 (x 4 for pyrUp) with BORDER_REFLECT_101,
//     pyrDown to ((w + 1) / 2, (h + 1) / 2), pyrUp to an explicit size by zero injection then the filter.  Evaluation
//     order: per source row a horizontal 5-tap sum left to right (k0 s0 + k1 s1 + ... + k4 s4, each step rounded), then the
//     vertical 5-tap sum of those row sums top to bottom in the same order, then the scale (1 / 256 or 1 / 64, exact).
//   the distance: the 3 x 3 DIST_L2 chamfer (a = 0.955, b = 1.3693) in integer units of 1e-4 (a = 9550, b = 13693,
//     exact), paths inside the tile; a tile without a boundary pixel is +inf everywhere.  float d = (float)(D / 1e4).
//   exp in the falloff: exp_restated, a double Taylor series after reduction by ln 2, rounded once to float.
//   Lab -> BGR8 (float path): Lab -> XYZ -> linear RGB as bgr8_from_lab8, clipped to [0, 1], encoded by srgb_encode8.
//   the colour table: vignetting always from model id 0 (readLayeredTileFromGeoTIFF never sets a sample's model id).
#pragma once

#include "ortho_layers.hpp"

#include <cstdint>
#include <vector>

namespace ochip_ob
{

using ochip_ol::lab_tables;
constexpr int MAX_LAYERS = ochip_ol::MAX_LAYERS;
constexpr int MAX_LEVELS = 16;
constexpr int MAX_TILE = 4096;
constexpr int32_t CH_A = 9550, CH_B = 13693; // the chamfer's steps in 1e-4 units
constexpr int32_t DIST_INF = 0x3FFFFFFF;      // no boundary pixel in the tile
constexpr uint32_t NONE = 0xFFFFFFFFu;

// One node id the layers may name, sorted by id: its camera record (NONE: not in the camera table) and its colour
// balance entry (has_color 0: none).  ochip.h's ochip_blend_id.
struct id_entry
{
    uint64_t id;
    uint32_t cam, has_color;
    double offset[3], brdf, slope[2];
};

OCHIP_OL int32_t find_id(const id_entry *t, uint32_t n, uint64_t id)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi) / 2;
        if (t[mid].id < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && t[lo].id == id ? (int32_t)lo : -1;
}

// ---- exp and the falloff --------------------------------------------------------------------------------------------

// expf restated: k = rint(x / ln 2), r = x - k ln 2 (ln 2 split in two, k ln2_hi exact), e^r by its Taylor series to
// r^20 (Horner), scaled by 2^k, rounded once to float.
OCHIP_OL float exp_restated(float xf)
{
    const double x = xf;
    if (x != x)
        return xf;
    if (x >= 100.0)
        return INFINITY;
    if (x <= -110.0)
        return 0.0f;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double k = rint(x / 0.6931471805599453);
    const double r = (x - k * ln2_hi) - k * ln2_lo;
    double p = 1.0;
    for (int n = 20; n >= 1; n--)
        p = 1.0 + r * p / (double)n;
    return (float)ldexp(p, (int)k);
}

// 2 / (1 + exp(steepness d)); d = +inf gives 0
OCHIP_OL float falloff(float steepness, float d)
{
    return 2.0f / (1.0f + exp_restated(steepness * d));
}

// ---- Lab -> BGR8 (float path) ---------------------------------------------------------------------------------------

// cv::COLOR_Lab2BGR on CV_32FC3 then convertTo(CV_8U, 255), restated: the documented Lab -> XYZ -> linear RGB, each
// channel clipped to [0, 1] and encoded by the threshold search (srgb_encode8; the clip does not change its answer)
OCHIP_OL void bgr8_from_labf(const lab_tables &T, const float lab[3], uint8_t bgr[3])
{
    const double L = lab[0], a = lab[1], b = lab[2];
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
    const double X = ochip_ol::lab_f_inv(fy + a / 500.0) * 0.950456;
    const double Z = ochip_ol::lab_f_inv(fy - b / 200.0) * 1.088754;
    double rgb[3] = {3.240479 * X - 1.53715 * Y - 0.498535 * Z, -0.969256 * X + 1.875991 * Y + 0.041556 * Z,
                     0.055648 * X - 0.204043 * Y + 1.057311 * Z};
    for (double &v : rgb)
        v = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
    bgr[0] = ochip_ol::srgb_encode8(T, rgb[2]);
    bgr[1] = ochip_ol::srgb_encode8(T, rgb[1]);
    bgr[2] = ochip_ol::srgb_encode8(T, rgb[0]);
}

OCHIP_OL float clampf(float v, float lo, float hi)
{
    return v < lo ? lo : hi < v ? hi : v; // std::clamp
}

// ---- one pixel's samples (ortho.cpp:1770-1876) ----------------------------------------------------------------------

// The band: inputs (ochip_ortho_layers' outputs and the DSM) and the per-pixel planes of the blend, [L][px] each.
struct band_view
{
    int L;
    int32_t cols;
    int64_t rows, row0;
    double min_x, max_y, gsd;
    const uint8_t *bgra; // [L][px][4]
    const uint64_t *id;  // [L][px]
    const float *dsm;    // [px]
    uint8_t *valid;      // [L][px]: alpha > 0 and not behind the camera
    float *weight;       // [L][px]: the recomputed weight, before the falloff
    float *lab;          // [L][px][3]: the corrected Lab
    int32_t *dist;       // [px]: the chamfer distance in 1e-4 units
};

struct color_model0
{
    int has;
    double vig[3];
};

// the plain image_from_3d (distort_keypoints.hpp:44-86, PLANAR) with R_inv; returns R_inv (p - position)'s z
OCHIP_OL double project_plain(const double *cam, double x, double y, double z, double pixel[2])
{
    const double d[3] = {x - cam[0], y - cam[1], z - cam[2]};
    const double *R = cam + 3;
    double ray[3];
    for (int i = 0; i < 3; i++)
        ray[i] = R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2];
    const double zc = ray[2] < 1e-3 ? 1e-3 : ray[2];
    const double p[2] = {ray[0] / zc, ray[1] / zc};
    const double *m = cam + 12; // f ppx ppy k1 k2 k3 p1 p2
    double r2[3];
    r2[0] = p[0] * p[0] + p[1] * p[1];
    r2[1] = r2[0] * r2[0];
    r2[2] = r2[1] * r2[0];
    const double radial = m[3] * r2[0] + m[4] * r2[1] + m[5] * r2[2];
    const double prod = p[0] * p[1];
    for (int i = 0; i < 2; i++)
    {
        const double dd = (1.0 + radial) * p[i] + m[6 + i] * (2.0 * prod) + m[7 - i] * (r2[0] + 2.0 * p[i] * p[i]);
        pixel[i] = m[0] * dd + m[1 + i];
    }
    return ray[2];
}

// Pixel i (band-local row r, column c) of every layer: validity, the recomputed weight and fields, float Lab and its
// correction.  A valid sample whose height is NaN or whose id has no camera keeps black, weight 0 and zero fields, as the
// reference's `continue` leaves them; one behind its camera turns invalid.
OCHIP_OL void prep_pixel(const lab_tables &T, const band_view &B, const double *cams, const id_entry *ids, uint32_t n_ids,
                         const color_model0 &M0, int64_t r, int32_t c)
{
    const size_t px = (size_t)B.rows * (size_t)B.cols, i = (size_t)r * (size_t)B.cols + (size_t)c;
    const double x = c * B.gsd + B.min_x;
    const double y = B.max_y - (B.row0 + r) * B.gsd;
    const float zf = B.dsm[i];
    for (int l = 0; l < B.L; l++)
    {
        const size_t o = (size_t)l * px + i;
        const uint8_t *s = B.bgra + 4 * o;
        bool valid = s[3] > 0;
        uint8_t bgr[3] = {0, 0, 0};
        float w = 0.0f, nr = 0.0f, nx = 0.0f, ny = 0.0f, va = 0.0f;
        const int32_t k = valid ? find_id(ids, n_ids, B.id[o]) : -1;
        if (valid && zf == zf && k >= 0 && ids[k].cam != NONE)
        {
            const double *cam = cams + (size_t)ids[k].cam * ochip_ol::CAM_DOUBLES;
            const double z = zf;
            double pixel[2];
            if (project_plain(cam, x, y, z, pixel) <= 0)
                valid = false;
            else
            {
                const int cols = (int)cam[20], rows = (int)cam[21];
                nr = ochip_ol::normalized_radius(pixel[0], pixel[1], cols, rows);
                ochip_ol::normalized_position(pixel[0], pixel[1], cols, rows, &nx, &ny);
                const double t[3] = {x - cam[0], y - cam[1], z - cam[2]};
                const double norm = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
                double cosang = norm > 0 ? cam[22] * (t[0] / norm) + cam[23] * (t[1] / norm) + cam[24] * (t[2] / norm)
                                         : cam[22] * t[0] + cam[23] * t[1] + cam[24] * t[2];
                cosang = cosang < -1.0 ? -1.0 : cosang > 1.0 ? 1.0 : cosang;
                va = (float)ochip_ol::acos_restated(cosang);
                w = ochip_ol::blend_weight((float)pixel[0], (float)pixel[1], cols, rows, (float)norm);
                bgr[0] = s[0], bgr[1] = s[1], bgr[2] = s[2];
            }
        }
        float lab[3];
        ochip_ol::labf_from_bgr8(T, bgr, lab);
        if (valid && k >= 0 && ids[k].has_color)
        {
            const id_entry &e = ids[k];
            lab[0] = lab[0] - (float)e.offset[0];
            lab[1] = lab[1] - (float)e.offset[1];
            lab[2] = lab[2] - (float)e.offset[2];
            if (M0.has)
            {
                const float r2 = nr * nr;
                const float vig = (float)M0.vig[0] * r2 + (float)M0.vig[1] * r2 * r2 + (float)M0.vig[2] * r2 * r2 * r2;
                lab[0] = lab[0] - vig;
            }
            lab[0] = lab[0] - (float)e.brdf * va * va;
            lab[0] = lab[0] - ((float)e.slope[0] * nx + (float)e.slope[1] * ny);
            lab[0] = clampf(lab[0], 0.0f, 100.0f);
            lab[1] = clampf(lab[1], -127.0f, 127.0f);
            lab[2] = clampf(lab[2], -127.0f, 127.0f);
        }
        B.valid[o] = valid ? 1 : 0;
        B.weight[o] = w;
        B.lab[3 * o] = lab[0], B.lab[3 * o + 1] = lab[1], B.lab[3 * o + 2] = lab[2];
    }
}

// ---- tiles, pyramid levels and the arena ----------------------------------------------------------------------------

// One output tile of the band and its pyramid in the arena: levels lf of the pull-push fill (fillInvalidRegions' count,
// the most), p of the blend (laplacianBlend's clamp); level l is lw x lh pixels at arena pixel loff[l].
struct tile_info
{
    int64_t r0, off;
    int32_t c0, tw, th, lf, p, pad;
    int32_t lw[MAX_LEVELS], lh[MAX_LEVELS];
    int64_t loff[MAX_LEVELS];
};

OCHIP_OL int fill_levels(int w, int h)
{
    const int m = w < h ? w : h;
    int l = 1;
    while ((m >> l) >= 2)
        l++;
    return l;
}

// the tiles of a band (rows x cols, tile size T) row-major; returns the arena's pixels (host)
inline int64_t tiles_build(int T, int64_t rows, int32_t cols, int pyramid_levels, std::vector<tile_info> *out)
{
    int64_t off = 0;
    out->clear();
    for (int64_t r0 = 0; r0 < rows; r0 += T)
        for (int32_t c0 = 0; c0 < cols; c0 += T)
        {
            tile_info t{};
            t.r0 = r0, t.c0 = c0;
            t.th = (int32_t)(rows - r0 < T ? rows - r0 : T);
            t.tw = cols - c0 < T ? cols - c0 : T;
            t.lf = fill_levels(t.tw, t.th);
            int p = 1;
            while (p < t.lf && p < pyramid_levels)
                p++;
            t.p = p;
            t.off = off;
            int w = t.tw, h = t.th;
            for (int l = 0; l < t.lf; l++)
            {
                t.lw[l] = w, t.lh[l] = h, t.loff[l] = off;
                off += (int64_t)w * h;
                w = (w + 1) / 2, h = (h + 1) / 2;
            }
            out->push_back(t);
        }
    return off;
}

// The band's pyramids: n arena pixels per layer.  wr: the weight pyramid ([L][n]; level 0 the normalised weight, the
// levels above pyrDown's, not renormalised); wc: colour x weight; fl: the pull-push fill; g: the colour's Gaussian
// pyramid ([L][n][3] each); bl: the blended Laplacian pyramid, reconstructed in place ([n][3]).
struct arena
{
    int L;
    int64_t n;
    float *wr, *wc, *fl, *g, *bl;
};

// ---- pyrDown / pyrUp ------------------------------------------------------------------------------------------------

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
OCHIP_OL int reflect101(int p, int len)
{
    if (len == 1)
        return 0;
    while (p < 0 || p >= len)
        p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

// pyrDown's pixel (x, y) of a w x h image of C interleaved channels
template <int C> OCHIP_OL void pyr_down_px(const float *src, int w, int h, int x, int y, float *out)
{
    const float k[5] = {1.0f, 4.0f, 6.0f, 4.0f, 1.0f};
    int xs[5];
    for (int j = 0; j < 5; j++)
        xs[j] = reflect101(2 * x + j - 2, w);
    float v[C] = {};
    for (int i = 0; i < 5; i++)
    {
        const float *row = src + (size_t)reflect101(2 * y + i - 2, h) * (size_t)w * C;
        for (int ch = 0; ch < C; ch++)
        {
            float s = k[0] * row[xs[0] * C + ch];
            for (int j = 1; j < 5; j++)
                s = s + k[j] * row[xs[j] * C + ch];
            v[ch] = i == 0 ? k[0] * s : v[ch] + k[i] * s;
        }
    }
    for (int ch = 0; ch < C; ch++)
        out[ch] = v[ch] * (1.0f / 256.0f);
}

// pyrUp's pixel (x, y) of the W x H result from a w x h image (W in {2w - 1, 2w}, H likewise): the zero-injected W x H
// image (source pixel (i, j) at (2i, 2j)) filtered with the kernel x 4
template <int C> OCHIP_OL void pyr_up_px(const float *src, int w, int W, int H, int x, int y, float *out)
{
    const float k[5] = {1.0f, 4.0f, 6.0f, 4.0f, 1.0f};
    int xs[5];
    for (int j = 0; j < 5; j++)
        xs[j] = reflect101(x + j - 2, W);
    float v[C] = {};
    for (int i = 0; i < 5; i++)
    {
        const int uy = reflect101(y + i - 2, H);
        const float *row = src + (size_t)(uy / 2) * (size_t)w * C;
        for (int ch = 0; ch < C; ch++)
        {
            float s = 0.0f;
            for (int j = 0; j < 5; j++)
            {
                const float u = (uy % 2 == 0 && xs[j] % 2 == 0) ? row[(xs[j] / 2) * C + ch] : 0.0f;
                s = j == 0 ? k[0] * u : s + k[j] * u;
            }
            v[ch] = i == 0 ? k[0] * s : v[ch] + k[i] * s;
        }
    }
    for (int ch = 0; ch < C; ch++)
        out[ch] = v[ch] * (4.0f / 256.0f);
}

// ---- the boundary mask and the chamfer ------------------------------------------------------------------------------

// a layer-0 valid pixel with a 4-neighbour inside its tile that is invalid or has another layer-0 camera
OCHIP_OL bool boundary_px(const band_view &B, const tile_info &t, int32_t lr, int32_t lc)
{
    const size_t i = (size_t)(t.r0 + lr) * (size_t)B.cols + (size_t)(t.c0 + lc);
    if (!B.valid[i])
        return false;
    const int dr[4] = {0, 0, -1, 1}, dc[4] = {-1, 1, 0, 0};
    for (int d = 0; d < 4; d++)
    {
        const int32_t nr = lr + dr[d], nc = lc + dc[d];
        if (nr >= 0 && nr < t.th && nc >= 0 && nc < t.tw)
        {
            const size_t j = (size_t)(t.r0 + nr) * (size_t)B.cols + (size_t)(t.c0 + nc);
            if (!B.valid[j] || B.id[j] != B.id[i])
                return true;
        }
    }
    return false;
}

OCHIP_OL int32_t mini(int32_t a, int32_t b)
{
    return b < a ? b : a;
}

// the two-pass chamfer of a th x tw tile, sequentially (the CPU route): src(r, c) true at a boundary pixel, D(r, c) the
// distance's int32_t in 1e-4 units
template <class Src, class Dst> inline void chamfer_seq(int32_t th, int32_t tw, Src src, Dst D)
{
    for (int32_t r = 0; r < th; r++)
        for (int32_t c = 0; c < tw; c++)
        {
            int32_t v = src(r, c) ? 0 : DIST_INF;
            if (r > 0)
            {
                v = mini(v, D(r - 1, c) + CH_A);
                if (c > 0)
                    v = mini(v, D(r - 1, c - 1) + CH_B);
                if (c < tw - 1)
                    v = mini(v, D(r - 1, c + 1) + CH_B);
            }
            if (c > 0)
                v = mini(v, D(r, c - 1) + CH_A);
            D(r, c) = mini(v, DIST_INF);
        }
    for (int32_t r = th - 1; r >= 0; r--)
        for (int32_t c = tw - 1; c >= 0; c--)
        {
            int32_t v = D(r, c);
            if (r < th - 1)
            {
                v = mini(v, D(r + 1, c) + CH_A);
                if (c > 0)
                    v = mini(v, D(r + 1, c - 1) + CH_B);
                if (c < tw - 1)
                    v = mini(v, D(r + 1, c + 1) + CH_B);
            }
            if (c < tw - 1)
                v = mini(v, D(r, c + 1) + CH_A);
            D(r, c) = mini(v, DIST_INF);
        }
}

inline void chamfer_tile(const band_view &B, const tile_info &t)
{
    chamfer_seq(
        t.th, t.tw, [&](int32_t r, int32_t c) { return boundary_px(B, t, r, c); },
        [&](int32_t r, int32_t c) -> int32_t & { return B.dist[(size_t)(t.r0 + r) * (size_t)B.cols + (size_t)(t.c0 + c)]; });
}

OCHIP_OL float dist_float(int32_t D)
{
    return D >= DIST_INF ? INFINITY : (float)((double)D / 10000.0);
}

// ---- the blend's steps, one output pixel each -----------------------------------------------------------------------

// the partition of unity and level 0 of wr and wc at arena pixel a: w [L] the weights (after the falloff), lab + l *
// lab_stride layer l's Lab
OCHIP_OL void unity_px(const arena &A, int64_t a, const float *w, const float *lab, size_t lab_stride)
{
    float sum = 0.0f;
    for (int l = 0; l < A.L; l++)
        sum = sum + w[l];
    sum = sum < 1e-6f ? 1e-6f : sum;
    for (int l = 0; l < A.L; l++)
    {
        const float nw = w[l] / sum;
        A.wr[(size_t)l * A.n + a] = nw;
        float *wc = A.wc + 3 * ((size_t)l * A.n + a);
        for (int ch = 0; ch < 3; ch++)
            wc[ch] = lab[l * lab_stride + ch] * nw;
    }
}

// the falloff on layers >= 1, then unity_px (band-local pixel r, c of tile t)
OCHIP_OL void weights_px(const band_view &B, const arena &A, const tile_info &t, float steepness, int64_t r, int32_t c)
{
    const size_t px = (size_t)B.rows * (size_t)B.cols, i = (size_t)r * (size_t)B.cols + (size_t)c;
    const float f = falloff(steepness, dist_float(B.dist[i]));
    float w[MAX_LAYERS];
    for (int l = 0; l < B.L; l++)
    {
        w[l] = B.weight[(size_t)l * px + i];
        if (l >= 1)
            w[l] = w[l] * f;
    }
    unity_px(A, t.off + (r - t.r0) * t.tw + (c - t.c0), w, B.lab + 3 * i, 3 * px);
}

// fillInvalidRegions' pyrDowns: level lv of wc and wr of layer l (1 <= lv < lf)
OCHIP_OL void fill_down_px(const arena &A, const tile_info &t, int l, int lv, int x, int y)
{
    const int w = t.lw[lv - 1], h = t.lh[lv - 1];
    const size_t at = (size_t)t.loff[lv] + (size_t)y * t.lw[lv] + x;
    pyr_down_px<3>(A.wc + 3 * ((size_t)l * A.n + t.loff[lv - 1]), w, h, x, y, A.wc + 3 * ((size_t)l * A.n + at));
    pyr_down_px<1>(A.wr + (size_t)l * A.n + t.loff[lv - 1], w, h, x, y, A.wr + (size_t)l * A.n + at);
}

// the pull back up: level lv of fl (the coarsest level lf - 1 first); level 0 also starts the Gaussian pyramid g
OCHIP_OL void fill_up_px(const arena &A, const tile_info &t, int l, int lv, int x, int y)
{
    const size_t at = (size_t)l * A.n + (size_t)t.loff[lv] + (size_t)y * t.lw[lv] + x;
    const float w = A.wr[at];
    const float d = w < 1e-6f ? 1e-6f : w;
    float v[3];
    if (lv == t.lf - 1 || w > 1e-6f)
        for (int ch = 0; ch < 3; ch++)
            v[ch] = A.wc[3 * at + ch] / d;
    else
        pyr_up_px<3>(A.fl + 3 * ((size_t)l * A.n + t.loff[lv + 1]), t.lw[lv + 1], t.lw[lv], t.lh[lv], x, y, v);
    for (int ch = 0; ch < 3; ch++)
    {
        A.fl[3 * at + ch] = v[ch];
        if (lv == 0)
            A.g[3 * at + ch] = v[ch];
    }
}

// the Gaussian pyramid of the filled colour: level lv of g (1 <= lv < p)
OCHIP_OL void gauss_down_px(const arena &A, const tile_info &t, int l, int lv, int x, int y)
{
    const size_t at = (size_t)t.loff[lv] + (size_t)y * t.lw[lv] + x;
    pyr_down_px<3>(A.g + 3 * ((size_t)l * A.n + t.loff[lv - 1]), t.lw[lv - 1], t.lh[lv - 1], x, y,
                   A.g + 3 * ((size_t)l * A.n + at));
}

// level lv of the blended Laplacian pyramid: the layers' Laplacian (the coarsest level: Gaussian) times their weight
// renormalised per level (level 0 as normalised), summed from zero in layer order
OCHIP_OL void blend_px(const arena &A, const tile_info &t, int lv, int x, int y)
{
    const size_t at = (size_t)t.loff[lv] + (size_t)y * t.lw[lv] + x;
    float level_sum = 0.0f;
    if (lv > 0)
    {
        for (int l = 0; l < A.L; l++)
            level_sum = level_sum + A.wr[(size_t)l * A.n + at];
        level_sum = level_sum < 1e-6f ? 1e-6f : level_sum;
    }
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < A.L; l++)
    {
        const float *g = A.g + 3 * ((size_t)l * A.n + at);
        float lap[3] = {g[0], g[1], g[2]};
        if (lv < t.p - 1)
        {
            float up[3];
            pyr_up_px<3>(A.g + 3 * ((size_t)l * A.n + t.loff[lv + 1]), t.lw[lv + 1], t.lw[lv], t.lh[lv], x, y, up);
            for (int ch = 0; ch < 3; ch++)
                lap[ch] = lap[ch] - up[ch];
        }
        const float wr = A.wr[(size_t)l * A.n + at];
        const float w = lv > 0 ? wr / level_sum : wr;
        for (int ch = 0; ch < 3; ch++)
            acc[ch] = acc[ch] + lap[ch] * w;
    }
    for (int ch = 0; ch < 3; ch++)
        A.bl[3 * at + ch] = acc[ch];
}

// the reconstruction, level lv (< p - 1) in place: pyrUp(level lv + 1) + level lv
OCHIP_OL void recon_px(const arena &A, const tile_info &t, int lv, int x, int y)
{
    const size_t at = (size_t)t.loff[lv] + (size_t)y * t.lw[lv] + x;
    float up[3];
    pyr_up_px<3>(A.bl + 3 * (size_t)t.loff[lv + 1], t.lw[lv + 1], t.lw[lv], t.lh[lv], x, y, up);
    for (int ch = 0; ch < 3; ch++)
        A.bl[3 * at + ch] = up[ch] + A.bl[3 * at + ch];
}

// laplacianBlend's colour at arena pixel a: the reconstruction clamped, Lab -> BGR8
OCHIP_OL void blended_bgr8(const lab_tables &T, const arena &A, size_t a, uint8_t bgr[3])
{
    const float *v = A.bl + 3 * a;
    const float lab[3] = {clampf(v[0], 0.0f, 100.0f), clampf(v[1], -127.0f, 127.0f), clampf(v[2], -127.0f, 127.0f)};
    bgr8_from_labf(T, lab, bgr);
}

// the output pixel (band-local r, c): clamped Lab -> BGR8 -> RGBA, or the checkerboard where no layer is valid
OCHIP_OL void final_px(const lab_tables &T, const band_view &B, const arena &A, const tile_info &t, int64_t r, int32_t c,
                       uint8_t *rgba)
{
    const size_t px = (size_t)B.rows * (size_t)B.cols, i = (size_t)r * (size_t)B.cols + (size_t)c;
    bool any = false;
    for (int l = 0; l < B.L; l++)
        any = any || B.valid[(size_t)l * px + i];
    uint8_t *o = rgba + 4 * i;
    if (!any)
    {
        const uint8_t grey = (B.row0 + r + c) % 2 == 0 ? 64 : 128;
        o[0] = o[1] = o[2] = grey;
        o[3] = 0;
        return;
    }
    uint8_t bgr[3];
    blended_bgr8(T, A, (size_t)t.off + (size_t)(r - t.r0) * t.tw + (size_t)(c - t.c0), bgr);
    o[0] = bgr[2], o[1] = bgr[1], o[2] = bgr[0], o[3] = 255;
}

} // namespace ochip_ob
