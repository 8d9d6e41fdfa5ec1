// AKAZE's schedule as data: the level table (AKAZEFeatures::Allocate_Memory_Evolution), the FED cycles, and for one
// call the form of every launch and the planes it reads and writes.  Plain C++17 without a HIP header and without
// getenv: akaze_run reads the environment and passes values in, the stage functions of akaze.hip execute what the plan says, and
// tests/akaze_plan_driver.cpp walks it on the CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ochip
{
namespace akaze
{

struct level_info
{
    int octave, w, h, sigma_size;
    float esigma;
    size_t off; // plane offset (floats) inside one image's pyramid
    int tile_off, tiles_x; // first id and row length of the level's 64 x 24 detection tiles
    int mask_off;          // first word of the level's maxima bit mask (one 64-bit word per row of a tile column)
    int sup_off, sup_tx;   // the suppression's masks: first word and words per row of the level's 8 x 8-pixel mask words
};

struct levels_dev
{
    int n;
    level_info l[16];
};

constexpr int BT_X = 64, BT_Y = 32; // blur tiles
constexpr int DT_Y = 24;             // detection tiles are 64 x 24 (16, 24, 32 rows measured: 43, 39, 40 us per image for the determinant kernels)
constexpr int FED_FUSE = 4;          // explicit diffusion steps per launch, at most

// the scale space's constants (cv::AKAZE's defaults, as the reference asks for them)
constexpr int OCTAVE_MAX = 4, SUBLEVELS = 4;
constexpr float SIGMA_OFFSET = 1.6f, DERIVATIVE_FACTOR = 1.5f, DET_THRESHOLD = 0.00005f;

// Which form pays depends on how many strips a launch has: a strip is one wavefront walking 40 - 90 rows, and a level of
// 400 x 300 pixels x 100 images is 2 400 of them on 1 024 SIMDs (level kernel: 150 us per launch against the tile kernels'
// 75; 200 x 150: 150 against 30) - the strips take the levels of >= this many pixels per launch (the first two octaves of
// a chunk of the bench), the tiles the rest
constexpr size_t STRIP_MIN_PIXELS = (size_t)32 << 20;

inline std::vector<float> gaussian_taps(float sigma)
{
    int ksize = (int)std::ceil(2.0f * (1.0f + (sigma - 0.8f) / 0.3f));
    if ((ksize % 2) == 0)
        ksize += 1;
    if (ksize < 1)
        ksize = 1;
    std::vector<double> k(ksize);
    double sum = 0;
    const int r = ksize / 2;
    for (int i = 0; i < ksize; i++)
    {
        const double x = i - r;
        k[i] = std::exp(-0.5 * x * x / ((double)sigma * sigma));
        sum += k[i];
    }
    std::vector<float> out(ksize);
    for (int i = 0; i < ksize; i++)
        out[i] = (float)(k[i] / sum);
    return out;
}

inline bool is_prime(int n)
{
    if (n < 2)
        return false;
    for (int d = 2; d * d <= n; d++)
        if (n % d == 0)
            return false;
    return true;
}

inline std::vector<float> fed_taus(float T, float tau_max) // FED cycle for stopping time T, kappa-cycle reordering
{
    const double pi = 3.14159265358979323846;
    const double t = (double)T;
    const int n = (int)(std::ceil(std::sqrt(3.0 * t / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5);
    std::vector<float> tau;
    if (n <= 0)
        return tau;
    const double scale = 3.0 * t / (tau_max * (double)(n * (n + 1)));
    const double c = 1.0 / (4.0 * n + 2.0), d = scale * tau_max / 2.0;
    std::vector<double> tauh(n);
    for (int k = 0; k < n; k++)
    {
        const double hh = std::cos(pi * (2.0 * k + 1.0) * c);
        tauh[k] = d / (hh * hh);
    }
    tau.resize(n);
    const int kappa = n / 2;
    int prime = n + 1;
    while (!is_prime(prime))
        prime++;
    for (int k = 0, l = 0; l < n; ++k, ++l)
    {
        int index = 0;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n)
            k++;
        tau[l] = (float)tauh[index];
    }
    return tau;
}

// The level table of a working size: what depends on the image shape alone (the buffers are sized from it).
struct level_table
{
    levels_dev LV{};
    std::vector<std::vector<float>> tsteps; // a level's FED step sizes (level 0: none)
    size_t img_stride = 0;                  // floats of one image's pyramid
    int n_tiles = 0;                        // detection tiles of one image
    size_t mask_stride = 0;                 // words of one image's maxima bit masks
    size_t sup_stride = 0;                  // words of one image's masks of the suppression (8 x 8 pixels per word)

    level_table(int W, int H)
    {
        std::vector<float> etime;
        for (int i = 0; i < OCTAVE_MAX; i++)
        {
            const float rfactor = 1.0f / (float)(1 << i);
            const int lw = (int)(W * rfactor), lh = (int)(H * rfactor);
            if ((lw < 80 || lh < 40) && i != 0) // (Allocate_Memory_Evolution: "smallest possible octave" - 80 wide, 40 high)
                break;
            for (int j = 0; j < SUBLEVELS; j++)
            {
                level_info &l = LV.l[LV.n++];
                l.octave = i;
                l.w = lw;
                l.h = lh;
                l.esigma = SIGMA_OFFSET * std::pow(2.0f, (float)j / (float)SUBLEVELS + (float)i);
                l.sigma_size = (int)std::lrintf(l.esigma * DERIVATIVE_FACTOR / (float)(1 << i));
                l.off = img_stride;
                img_stride += (size_t)lw * lh;
                l.tiles_x = (lw + BT_X - 1) / BT_X;
                l.tile_off = n_tiles;
                n_tiles += l.tiles_x * ((lh + DT_Y - 1) / DT_Y);
                l.mask_off = (int)mask_stride;
                mask_stride += (size_t)l.tiles_x * lh;
                l.sup_off = (int)sup_stride;
                l.sup_tx = (lw + 7) / 8;
                sup_stride += (size_t)l.sup_tx * ((lh + 7) / 8);
                etime.push_back(0.5f * (l.esigma * l.esigma));
            }
        }
        tsteps.resize(LV.n);
        for (int i = 1; i < LV.n; i++)
            tsteps[i] = fed_taus(etime[i] - etime[i - 1], 0.25f);
    }
};

// the columns [x0, x1] / rows [y0, y1] whose descriptor window [round(x - margin) - 1, round(x + margin) + 1] stays inside
// the level (the predicate det_maxima_kernel evaluates per pixel: an interval in x and in y; empty: lo > hi)
struct det_window_t
{
    int x0 = 1, x1 = 0, y0 = 1, y1 = 0;
};
inline float det_margin(const level_info &l)
{
    return (10.0f * std::sqrt(2.0f)) * (float)l.sigma_size; // descriptor window half width, M-LDB
}
inline det_window_t det_window(const level_info &l)
{
    const float margin = det_margin(l);
    det_window_t win;
    auto span = [&](int n, int *lo, int *hi) {
        bool any = false;
        for (int v = 1; v < n - 1; v++)
            if ((int)std::rint((float)v - margin) - 1 >= 0 && (int)std::rint((float)v + margin) + 1 < n)
            {
                if (!any)
                    *lo = v;
                *hi = v;
                any = true;
            }
    };
    span(l.w, &win.x0, &win.x1);
    span(l.h, &win.y0, &win.y1);
    return win;
}

// ---- one call's plan

struct plan_inputs
{
    uint32_t B = 1;                                                             // images per launch
    bool tile_levels = false, tile_det = false, strip_levels = false, strip_det = false; // OCHIP_TEST_HOOKS
    size_t strip_min_pixels = STRIP_MIN_PIXELS; // OCHIP_STRIP_MIN_PIXELS (the tests lower it: a small batch then takes a bench chunk's mixed route)
    bool aligned16 = true;  // the working image, the pyramids and the two scratch planes start on 16-byte boundaries
    bool keep_flow = false; // OCHIP_DUMP_PLANES: every level leaves its conductivity plane behind
};

// a plane a launch reads or writes: level i's image Lt[i], the scratch plane the FED groups alternate with, or the
// conductivity plane
enum class plane_id
{
    none,
    level,
    ping,
    flow
};
struct plane_ref
{
    plane_id id = plane_id::none;
    int level = 0; // plane_id::level
    bool operator==(const plane_ref &o) const
    {
        return id == o.id && (id != plane_id::level || level == o.level);
    }
};

enum class launch_kind
{
    halfsample,      // the octave's first image: 2 x 2 means of the last level of the octave before
    halfsample_area, // the same with an odd dimension: cv::resize's general area path
    smooth,          // tiles: Lsmooth -> conductivity (dst = flow) and (Lx, Ly)
    strip,           // strips: the same and the level's first FED group behind them in one launch
    diffuse          // tiles: one FED group (reads flow too)
};
struct launch
{
    launch_kind kind;
    plane_ref src, dst;
    int first_step = 0, n_steps = 0; // strip, diffuse: the level's FED steps this launch takes
};

struct level_plan
{
    bool strip = false;         // register strips or LDS tiles (level 0, the base image, has tiles only)
    std::vector<int> groups;    // the FED steps in balanced groups of <= FED_FUSE
    std::vector<launch> launches;
    bool store_flow = false;    // strip: later launches of the level (or the dump) need the conductivity plane
    plane_ref half_out;         // strip: not none = the epilogue writes the next octave's first image there (and no half-sample launch follows)
    bool det_strip = false;     // the determinant + maxima pass as strips or tiles
    det_window_t det_win;
};

struct plan
{
    const char *error = nullptr; // not null: the table left what the kernels are instantiated for; nothing may be launched
    bool contrast_strip = false; // the contrast factor's gradient pass as strips or tiles
    bool det_accumulate = false; // strips may run: they add their maxima to zeroed masks and tile counts
    std::vector<level_plan> lv;
};

// The instantiated set: derivative scales 2 .. 4 everywhere, and a strip launch carries a first group of 3 or 4 steps.
inline bool instantiated(int sigma_size, int first_group)
{
    return sigma_size >= 2 && sigma_size <= 4 && (first_group == 3 || first_group == 4);
}

inline plan make_plan(const level_table &T, int W, int H, const plan_inputs &in)
{
    const levels_dev &LV = T.LV;
    plan P;
    P.lv.resize(LV.n);
    // the level's FED steps in balanced groups of <= FED_FUSE, a launch each (the first of a strip level rides in its launch)
    for (int i = 1; i < LV.n; i++)
    {
        const int n_steps = (int)T.tsteps[i].size(), n_groups = (n_steps + FED_FUSE - 1) / FED_FUSE;
        for (int g = 0; g < n_groups; g++)
            P.lv[i].groups.push_back(n_steps / n_groups + (g < n_steps % n_groups ? 1 : 0));
    }
    // what the launch code below and the kernels are instantiated for.  The constants above give, for levels 0 .. 15,
    // sigma_size 2 3 3 4 in every octave and 3 3 4 | 4 5 6 7 | 8 10 12 14 | 17 20 24 29 steps for levels 1 .. 15: a change of
    // SIGMA_OFFSET or SUBLEVELS that leaves this fails the call instead of launching nothing
    for (int i = 0; i < LV.n && !P.error; i++)
        if (LV.l[i].sigma_size < 2 || LV.l[i].sigma_size > 4)
            P.error = "akaze: a level's derivative scale is outside 2..4";
        else if (i > 0 && P.lv[i].groups.empty())
            P.error = "akaze: a level without FED steps";
        else if (i > 0 && !instantiated(LV.l[i].sigma_size, P.lv[i].groups[0]))
            P.error = "akaze: a level's first FED group is not of 3 or 4 steps";
    // (and the Gaussians of the levels and of the base image: 5 and 9 taps, the radii the tile kernels are instantiated with)
    if (!P.error && (gaussian_taps(1.0f).size() != 5 || gaussian_taps(SIGMA_OFFSET).size() != 9))
        P.error = "akaze: unexpected Gaussian kernel sizes";
    if (P.error)
        return P;

    // The register-strip kernels load pairs of pixels with 8 / 16-byte loads: even widths and plane offsets (every level of
    // an image whose working width is a multiple of 8; the tile kernels take the rest, and the hooks tile_det / tile_levels
    // all of it; strip_levels / strip_det: strips wherever they can, whatever the launch's size)
    const size_t plane0 = (size_t)W * H;
    auto pays = [&](int w, int h, bool forced, size_t threshold) { return forced || (size_t)w * h * in.B >= threshold; };
    // (the contrast pass - the level kernel's Gaussian and distance-1 pattern with the magnitude where the conductivity is -
    // keeps the built-in threshold: OCHIP_STRIP_MIN_PIXELS moves the levels and the determinant only)
    P.contrast_strip = !in.tile_levels && (W & 1) == 0 && (plane0 & 1) == 0 && W >= 64 && H >= 64 && in.aligned16 &&
                       pays(W, H, in.strip_levels, STRIP_MIN_PIXELS);
    bool det_strips = !in.tile_det && (T.img_stride & 1) == 0 && (plane0 & 1) == 0 && in.aligned16;
    for (int i = 0; i < LV.n; i++)
        det_strips = det_strips && (LV.l[i].w & 1) == 0 && (LV.l[i].off & 1) == 0 && LV.l[i].w >= 8 && LV.l[i].h >= 8;
    P.det_accumulate = det_strips;
    for (int i = 0; i < LV.n; i++)
    {
        const level_info &l = LV.l[i];
        P.lv[i].det_strip = det_strips && pays(l.w, l.h, in.strip_det, in.strip_min_pixels);
        P.lv[i].det_win = det_window(l);
        P.lv[i].strip = i > 0 && det_strips && !in.tile_levels && pays(l.w, l.h, in.strip_levels, in.strip_min_pixels) && l.w >= 64 && l.h >= 64;
    }

    // Where the launches of a level read and write.  A level starts from the previous level's image (half-sampled at a new
    // octave); its FED groups alternate between the level plane and the scratch plane so that the LAST one lands in the
    // level plane, and an octave's first image is put where the level's first group does not write.
    auto group_dst = [&](int i, int g) {
        const bool to_level = ((int)P.lv[i].groups.size() - 1 - g) % 2 == 0;
        return to_level ? plane_ref{plane_id::level, i} : plane_ref{plane_id::ping, 0};
    };
    auto new_octave = [&](int i) { return LV.l[i].octave > LV.l[i - 1].octave; };
    auto start_of = [&](int i) {
        if (!new_octave(i))
            return plane_ref{plane_id::level, i - 1};
        return group_dst(i, 0).id == plane_id::level ? plane_ref{plane_id::ping, 0} : plane_ref{plane_id::level, i};
    };
    for (int i = 1; i < LV.n; i++)
    {
        const level_info &l = LV.l[i], &p = LV.l[i - 1];
        level_plan &lp = P.lv[i];
        const int n_groups = (int)lp.groups.size();
        plane_ref src = start_of(i);
        if (new_octave(i))
        {
            if (p.w != 2 * l.w || p.h != 2 * l.h) // (an odd dimension: OpenCV's general area path, see halfsample_area_kernel)
                lp.launches.push_back({launch_kind::halfsample_area, {plane_id::level, i - 1}, src});
            else if (P.lv[i - 1].half_out.id == plane_id::none) // (else: the last level kernel of the octave before wrote it with its own rows)
                lp.launches.push_back({launch_kind::halfsample, {plane_id::level, i - 1}, src});
        }
        int g = 0, k = 0;
        if (lp.strip)
        {
            lp.launches.push_back({launch_kind::strip, src, group_dst(i, 0), 0, lp.groups[0]});
            src = group_dst(i, 0);
            k = lp.groups[0];
            g = 1;
            lp.store_flow = n_groups > 1 || in.keep_flow;
            // the octave's last level with its whole FED cycle in this launch: the next octave's first image - 2 x 2 means of
            // this level's final rows - leaves with them (halfsample_kernel read the level again: 2.5 us per image at the
            // first octave boundary)
            if (i + 1 < LV.n && new_octave(i + 1) && n_groups == 1 && l.w == 2 * LV.l[i + 1].w && l.h == 2 * LV.l[i + 1].h)
                lp.half_out = start_of(i + 1);
        }
        else
            lp.launches.push_back({launch_kind::smooth, src, {plane_id::flow, 0}});
        for (; g < n_groups; k += lp.groups[g], g++)
        {
            lp.launches.push_back({launch_kind::diffuse, src, group_dst(i, g), k, lp.groups[g]});
            src = group_dst(i, g);
        }
    }
    return P;
}

} // namespace akaze
} // namespace ochip
