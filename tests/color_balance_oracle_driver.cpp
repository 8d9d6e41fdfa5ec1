// Test infrastructure: the colour-balance problem posed on the oracle's restatement of Ceres (oracle/mini_ceres.hpp,
// oracle/relax_mini_ceres.cpp), block by block as solveColorBalance does (src/ortho/color_balance.cpp:57-148): the
// yardstick of tests/test_color_balance_host.py and of the recorded results under tests/golden/color_balance/.
//
//   color_balance_oracle_driver <problem file>
// Problem file (text): n, then n lines `camera_id_a camera_id_b model_id_a model_id_b` followed by the 14 floats
// lab_a[3] lab_b[3] radius_a radius_b angle_a angle_b nx_a ny_a nx_b ny_b, each as the hexadecimal of its 32 bits.
// Output: `summary <iterations> <usable> <initial_cost> <final_cost>`, `message <text>`, one `iteration` line per record
// (cost, cost_change, gradient_max_norm, step_norm, relative_decrease, radius, valid, successful), one `camera <id> <6
// values>` line per camera and one `model <id> <3 values>` line per model, ascending ids, all %.17g.
#include "../oracle/mini_ceres.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>

namespace mc = oracle::mc;

namespace
{

struct Corr
{
    uint64_t cam_a, cam_b;
    uint32_t model_a, model_b;
    float lab_a[3], lab_b[3], r_a, r_b, theta_a, theta_b, nx_a, ny_a, nx_b, ny_b;
};

// One side of a correspondence as the cost functors see it, and the observation it leaves after the radiometric model:
// every Lab channel loses the image's offset; the L channel also loses the vignetting polynomial in the squared
// normalised radius, the BRDF term in the squared view angle and the brightness slope over the normalised pixel
// position.  The squared radius and angle are products of floats, widened afterwards; their powers are formed in T
// (csrc/color_balance.hpp: eval_block keeps the same arithmetic).
struct Side
{
    float lab[3], radius, angle, nx, ny;
};

template <typename T> void corrected_lab(const Side &s, const T *offset, const T *brdf, const T *vig, const T *slope, T *out)
{
    const T rr = T(s.radius * s.radius), tt = T(s.angle * s.angle);
    const T lens_and_surface = vig[0] * rr + vig[1] * rr * rr + vig[2] * rr * rr * rr + brdf[0] * tt;
    const T tilt = slope[0] * T(s.nx) + slope[1] * T(s.ny);
    for (int k = 0; k < 3; k++)
        out[k] = T(s.lab[k]) - offset[k];
    out[0] -= lens_and_surface + tilt;
}

Side side_a(const Corr &c)
{
    return Side{{c.lab_a[0], c.lab_a[1], c.lab_a[2]}, c.r_a, c.theta_a, c.nx_a, c.ny_a};
}
Side side_b(const Corr &c)
{
    return Side{{c.lab_b[0], c.lab_b[1], c.lab_b[2]}, c.r_b, c.theta_b, c.nx_b, c.ny_b};
}

// The residual of a correspondence: what image a keeps of the point minus what image b keeps of it.  The two structs
// differ only in the parameter blocks Ceres is told about: a model shared by both images is one block, named once.
struct MatchCost // parameter blocks: off_a 3, brdf_a 1, vig_a 3, off_b 3, brdf_b 1, vig_b 3, slope_a 2, slope_b 2
{
    Corr c;
    template <typename T>
    bool operator()(const T *off_a, const T *brdf_a, const T *vig_a, const T *off_b, const T *brdf_b, const T *vig_b, const T *slope_a,
                    const T *slope_b, T *residuals) const
    {
        T a[3], b[3];
        corrected_lab(side_a(c), off_a, brdf_a, vig_a, slope_a, a);
        corrected_lab(side_b(c), off_b, brdf_b, vig_b, slope_b, b);
        for (int k = 0; k < 3; k++)
            residuals[k] = a[k] - b[k];
        return true;
    }
};

struct MatchCostSharedVig // off_a 3, brdf_a 1, off_b 3, brdf_b 1, vig 3, slope_a 2, slope_b 2
{
    Corr c;
    template <typename T>
    bool operator()(const T *off_a, const T *brdf_a, const T *off_b, const T *brdf_b, const T *vig, const T *slope_a, const T *slope_b,
                    T *residuals) const
    {
        T a[3], b[3];
        corrected_lab(side_a(c), off_a, brdf_a, vig, slope_a, a);
        corrected_lab(side_b(c), off_b, brdf_b, vig, slope_b, b);
        for (int k = 0; k < 3; k++)
            residuals[k] = a[k] - b[k];
        return true;
    }
};

template <int N> struct Prior // ExposurePrior / BRDFPrior / SlopePrior / VignettingPrior
{
    double weight;
    template <typename T> bool operator()(const T *x, T *residuals) const
    {
        for (int k = 0; k < N; k++)
            residuals[k] = T(weight) * x[k];
        return true;
    }
};

struct Image
{
    double off[3] = {0, 0, 0}, brdf = 0, slope[2] = {0, 0};
};
struct Model
{
    double vig[3] = {0, 0, 0};
};

float hex_float(const char *s)
{
    const uint32_t bits = (uint32_t)strtoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f)
        return 2;
    size_t n = 0;
    if (fscanf(f, "%zu", &n) != 1)
        return 2;
    std::vector<Corr> corr(n);
    for (auto &c : corr)
    {
        char h[14][16];
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %u %u", &c.cam_a, &c.cam_b, &c.model_a, &c.model_b) != 4)
            return 2;
        for (auto &s : h)
            if (fscanf(f, "%15s", s) != 1)
                return 2;
        for (int k = 0; k < 3; k++)
            c.lab_a[k] = hex_float(h[k]), c.lab_b[k] = hex_float(h[3 + k]);
        c.r_a = hex_float(h[6]), c.r_b = hex_float(h[7]), c.theta_a = hex_float(h[8]), c.theta_b = hex_float(h[9]);
        c.nx_a = hex_float(h[10]), c.ny_a = hex_float(h[11]), c.nx_b = hex_float(h[12]), c.ny_b = hex_float(h[13]);
    }
    fclose(f);

    // (std::map: node stability - the problem keeps pointers into the values - and ascending ids for the output)
    std::map<uint64_t, Image> images;
    std::map<uint32_t, Model> models;
    std::unordered_map<uint64_t, int> cam_count;
    std::unordered_map<uint32_t, int> model_count;
    for (const auto &c : corr)
    {
        images[c.cam_a], images[c.cam_b], models[c.model_a], models[c.model_b];
        cam_count[c.cam_a]++, cam_count[c.cam_b]++, model_count[c.model_a]++, model_count[c.model_b]++;
    }
    mc::Problem problem;
    const mc::HuberLoss huber(5.0);
    for (const auto &c : corr)
    {
        Image &a = images[c.cam_a], &b = images[c.cam_b];
        Model &va = models[c.model_a], &vb = models[c.model_b];
        if (c.model_a == c.model_b)
            problem.AddResidualBlock(new mc::AutoDiffCostFunction<MatchCostSharedVig, 3, 3, 1, 3, 1, 3, 2, 2>(new MatchCostSharedVig{c}),
                                     &huber, {a.off, &a.brdf, b.off, &b.brdf, va.vig, a.slope, b.slope});
        else
            problem.AddResidualBlock(new mc::AutoDiffCostFunction<MatchCost, 3, 3, 1, 3, 3, 1, 3, 2, 2>(new MatchCost{c}), &huber,
                                     {a.off, &a.brdf, va.vig, b.off, &b.brdf, vb.vig, a.slope, b.slope});
    }
    for (auto &[id, im] : images)
    {
        const double w = 0.1 * std::sqrt((double)std::max(1, cam_count[id]));
        problem.AddResidualBlock(new mc::AutoDiffCostFunction<Prior<3>, 3, 3>(new Prior<3>{w}), nullptr, {im.off});
        problem.AddResidualBlock(new mc::AutoDiffCostFunction<Prior<1>, 1, 1>(new Prior<1>{w}), nullptr, {&im.brdf});
        problem.AddResidualBlock(new mc::AutoDiffCostFunction<Prior<2>, 2, 2>(new Prior<2>{w}), nullptr, {im.slope});
    }
    for (auto &[id, m] : models)
    {
        const double w = 0.1 * std::sqrt((double)std::max(1, model_count[id]));
        problem.AddResidualBlock(new mc::AutoDiffCostFunction<Prior<3>, 3, 3>(new Prior<3>{w}), nullptr, {m.vig});
    }
    mc::SolverOptions options; // color_balance.cpp:140-148; everything else Ceres' default
    options.max_num_iterations = 20;
    options.function_tolerance = 1e-4;
    options.gradient_tolerance = 1e-6;
    options.parameter_tolerance = 1e-4;
    options.initial_trust_region_radius = 1e4;
    mc::SolverSummary summary;
    mc::Solve(options, &problem, &summary);
    printf("summary %zu %d %.17g %.17g\n", summary.iterations.size(), summary.usable ? 1 : 0, summary.initial_cost, summary.final_cost);
    printf("message %s\n", summary.message.c_str());
    for (const auto &it : summary.iterations)
        printf("iteration %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", it.cost, it.cost_change, it.gradient_max_norm, it.step_norm,
               it.relative_decrease, it.trust_region_radius, it.step_is_valid ? 1 : 0, it.step_is_successful ? 1 : 0);
    for (const auto &[id, im] : images)
        printf("camera %" PRIu64 " %.17g %.17g %.17g %.17g %.17g %.17g\n", id, im.off[0], im.off[1], im.off[2], im.brdf, im.slope[0],
               im.slope[1]);
    for (const auto &[id, m] : models)
        printf("model %u %.17g %.17g %.17g\n", id, m.vig[0], m.vig[1], m.vig[2]);
    return 0;
}
