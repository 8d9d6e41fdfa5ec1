// liboc_host.so: the colour-balance solve between the layered render and the blend (solveColorBalance,
// src/ortho/color_balance.cpp; its caller Pipeline::Impl::color_balance, src/pipeline/pipeline.cpp:987-1018): the id
// tables, the CPU route, the gauge removal and the C ABI of include/oc_host.h.
//
// The CPU route is the yardstick of the device route (color_balance.hip) and a usable path for small surveys: the same
// per-correspondence arithmetic (color_balance.hpp), the trust-region rules of ceres::TrustRegionMinimizer with
// LevenbergMarquardtStrategy (jacobi scaling, monotonic steps - what lm_solve restates on the device), sums in the
// order of the correspondences, and a plain Cholesky on the dense normal equations.  It holds J'J as a dense
// n x n matrix, n = 6 cameras + 3 models: CPU_MAX_UNKNOWNS bounds it.
#include "../../../include/oc_host.h"

#include "../color_balance.hpp"
#include "../color_balance_plan.hpp"
#include "capi_graph.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace
{

namespace cb = ochip_cb;

thread_local std::string cb_error;

constexpr size_t CPU_MAX_UNKNOWNS = 4096; // 128 MiB per dense matrix, three of them alive in a solve

// the solve's tables: sorted unique camera and model ids, per correspondence their rows, the appearance counts
struct tables
{
    std::vector<uint64_t> cam_ids;
    std::vector<uint32_t> model_ids;
    std::vector<uint32_t> cam_a, cam_b, model_a, model_b;
    std::vector<uint64_t> cam_count, model_count;
};

template <typename T> uint32_t row_of(const std::vector<T> &sorted, T id)
{
    return (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), id) - sorted.begin());
}

// ids == nullptr: collect them from the correspondences; else they are given (sorted, unique) and must hold every id
bool build_tables(const ochip_color_corr *corr, size_t n, const uint64_t *cam_ids, size_t n_cams, const uint32_t *model_ids,
                  size_t n_models, tables *t)
{
    if (cam_ids || model_ids)
    {
        t->cam_ids.assign(cam_ids, cam_ids + n_cams);
        t->model_ids.assign(model_ids, model_ids + n_models);
        for (size_t i = 1; i < n_cams; i++)
            if (!(cam_ids[i - 1] < cam_ids[i]))
                return cb_error = "camera ids must be sorted and unique", false;
        for (size_t i = 1; i < n_models; i++)
            if (!(model_ids[i - 1] < model_ids[i]))
                return cb_error = "model ids must be sorted and unique", false;
    }
    else
    {
        for (size_t i = 0; i < n; i++)
        {
            t->cam_ids.push_back(corr[i].camera_id_a), t->cam_ids.push_back(corr[i].camera_id_b);
            t->model_ids.push_back(corr[i].model_id_a), t->model_ids.push_back(corr[i].model_id_b);
        }
        std::sort(t->cam_ids.begin(), t->cam_ids.end());
        t->cam_ids.erase(std::unique(t->cam_ids.begin(), t->cam_ids.end()), t->cam_ids.end());
        std::sort(t->model_ids.begin(), t->model_ids.end());
        t->model_ids.erase(std::unique(t->model_ids.begin(), t->model_ids.end()), t->model_ids.end());
    }
    t->cam_a.resize(n), t->cam_b.resize(n), t->model_a.resize(n), t->model_b.resize(n);
    t->cam_count.assign(t->cam_ids.size(), 0), t->model_count.assign(t->model_ids.size(), 0);
    for (size_t i = 0; i < n; i++)
    {
        const uint32_t a = row_of(t->cam_ids, corr[i].camera_id_a), b = row_of(t->cam_ids, corr[i].camera_id_b);
        const uint32_t ma = row_of(t->model_ids, corr[i].model_id_a), mb = row_of(t->model_ids, corr[i].model_id_b);
        if (a >= t->cam_ids.size() || t->cam_ids[a] != corr[i].camera_id_a || b >= t->cam_ids.size() ||
            t->cam_ids[b] != corr[i].camera_id_b || ma >= t->model_ids.size() || t->model_ids[ma] != corr[i].model_id_a ||
            mb >= t->model_ids.size() || t->model_ids[mb] != corr[i].model_id_b)
            return cb_error = "a correspondence names an id that is not in the tables", false;
        if (a == b) // Ceres aborts on a residual block that names one parameter block twice
            return cb_error = "correspondence " + std::to_string(i) + " pairs camera " + std::to_string(corr[i].camera_id_a) +
                              " with itself",
                   false;
        t->cam_a[i] = a, t->cam_b[i] = b, t->model_a[i] = ma, t->model_b[i] = mb;
        t->cam_count[a]++, t->cam_count[b]++, t->model_count[ma]++, t->model_count[mb]++;
    }
    return true;
}

cb::obs obs_of(const ochip_color_corr &c)
{
    cb::obs o;
    for (int k = 0; k < 3; k++)
        o.lab[0][k] = c.lab_a[k], o.lab[1][k] = c.lab_b[k];
    o.radius[0] = c.normalized_radius_a, o.radius[1] = c.normalized_radius_b;
    o.angle[0] = c.view_angle_a, o.angle[1] = c.view_angle_b;
    o.nx[0] = c.normalized_x_a, o.nx[1] = c.normalized_x_b;
    o.ny[0] = c.normalized_y_a, o.ny[1] = c.normalized_y_b;
    return o;
}

// The CPU route's problem: unknowns in table order, camera i at 6 i, model m at 6 n_cams + 3 m
struct problem
{
    const ochip_color_corr *corr;
    size_t n_corr;
    const tables *t;
    size_t nc, nm, n;
    std::vector<double> weight; // per unknown: the prior's weight

    problem(const ochip_color_corr *c, size_t k, const tables *tb) : corr(c), n_corr(k), t(tb)
    {
        nc = t->cam_ids.size(), nm = t->model_ids.size();
        n = cb::CAM_UNKNOWNS * nc + cb::MODEL_UNKNOWNS * nm;
        weight.resize(n);
        for (size_t i = 0; i < nc; i++)
            for (int k2 = 0; k2 < cb::CAM_UNKNOWNS; k2++)
                weight[cb::CAM_UNKNOWNS * i + k2] = cb::prior_weight(t->cam_count[i]);
        for (size_t m = 0; m < nm; m++)
            for (int k2 = 0; k2 < cb::MODEL_UNKNOWNS; k2++)
                weight[cb::CAM_UNKNOWNS * nc + cb::MODEL_UNKNOWNS * m + k2] = cb::prior_weight(t->model_count[m]);
    }

    // cost, and (JtJ != nullptr) the full symmetric J'J (n x n) and J'r at x; false: a residual is not finite
    bool evaluate(const double *x, double *cost, double *JtJ, double *Jtr) const
    {
        if (JtJ)
        {
            std::fill(JtJ, JtJ + n * n, 0.0);
            std::fill(Jtr, Jtr + n, 0.0);
        }
        double total = 0;
        double J[3 * cb::BLOCK_COLS], res[3];
        for (size_t i = 0; i < n_corr; i++)
        {
            const uint32_t a = t->cam_a[i], b = t->cam_b[i], ma = t->model_a[i], mb = t->model_b[i];
            const bool flip = a > b, shared = ma == mb;
            const size_t va = cb::CAM_UNKNOWNS * nc + cb::MODEL_UNKNOWNS * ma, vb = cb::CAM_UNKNOWNS * nc + cb::MODEL_UNKNOWNS * mb;
            const double *const cam[2] = {x + cb::CAM_UNKNOWNS * a, x + cb::CAM_UNKNOWNS * b};
            const double *const vig[2] = {x + va, x + vb};
            double c = 0;
            if (!cb::eval_block(obs_of(corr[i]), cam, vig, shared, flip, res, JtJ ? J : nullptr, &c))
                return false;
            total += c;
            if (!JtJ)
                continue;
            size_t col[cb::BLOCK_COLS];
            for (int k = 0; k < cb::CAM_UNKNOWNS; k++)
            {
                col[k] = cb::CAM_UNKNOWNS * (flip ? b : a) + k;
                col[cb::CAM_UNKNOWNS + k] = cb::CAM_UNKNOWNS * (flip ? a : b) + k;
            }
            for (int k = 0; k < cb::MODEL_UNKNOWNS; k++)
            {
                col[12 + k] = (flip ? vb : va) + k;
                col[15 + k] = (flip ? va : vb) + k; // (shared: these columns of J are zero)
            }
            const int cols = shared ? 15 : cb::BLOCK_COLS;
            for (int p = 0; p < cols; p++)
            {
                Jtr[col[p]] += cb::jtr_entry(J, res, p);
                for (int q = 0; q <= p; q++)
                {
                    const double v = cb::jtj_entry(J, p, q);
                    JtJ[col[p] * n + col[q]] += v;
                    if (col[p] != col[q])
                        JtJ[col[q] * n + col[p]] += v;
                }
            }
        }
        for (size_t k = 0; k < n; k++) // ExposurePrior, BRDFPrior, SlopePrior, VignettingPrior: r = w x, no loss
        {
            const double r = weight[k] * x[k];
            total += 0.5 * (r * r);
            if (JtJ)
            {
                JtJ[k * n + k] += weight[k] * weight[k];
                Jtr[k] += weight[k] * r;
            }
        }
        *cost = total;
        return std::isfinite(total);
    }
};

// A x = b for the symmetric positive definite A (row-major, lower triangle read, destroyed), x into b; rows are
// walked inside their profile, which skips exact zeros only
bool cholesky_solve(std::vector<double> &A, std::vector<double> &b, size_t n)
{
    std::vector<size_t> first(n);
    for (size_t i = 0; i < n; i++)
    {
        size_t f = 0;
        while (f < i && A[i * n + f] == 0.0)
            f++;
        first[i] = f;
    }
    for (size_t j = 0; j < n; j++)
    {
        double d = A[j * n + j];
        for (size_t k = first[j]; k < j; k++)
            d -= A[j * n + k] * A[j * n + k];
        if (!(d > 0) || !std::isfinite(d))
            return false;
        d = std::sqrt(d);
        A[j * n + j] = d;
        for (size_t i = j + 1; i < n; i++)
        {
            if (first[i] > j)
                continue;
            double s = A[i * n + j];
            for (size_t k = std::max(first[i], first[j]); k < j; k++)
                s -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = s / d;
        }
    }
    for (size_t i = 0; i < n; i++)
    {
        double s = b[i];
        for (size_t k = first[i]; k < i; k++)
            s -= A[i * n + k] * b[k];
        b[i] = s / A[i * n + i];
    }
    for (size_t i = n; i-- > 0;)
    {
        b[i] /= A[i * n + i];
        for (size_t k = first[i]; k < i; k++)
            b[k] -= A[i * n + k] * b[i];
    }
    return true;
}

double norm2(const std::vector<double> &v)
{
    double s = 0;
    for (double e : v)
        s += e * e;
    return std::sqrt(s);
}

// ceres::Solve on the problem, TRUST_REGION / LEVENBERG_MARQUARDT with solveColorBalance's options
void solve_cpu(const problem &P, std::vector<double> &x, ochip_relax_summary *sum)
{
    const size_t n = P.n;
    *sum = ochip_relax_summary{};
    sum->num_parameters = (int)n;
    sum->num_residual_blocks = (int)(P.n_corr + 3 * P.nc + P.nm);
    std::vector<double> JtJ(n * n), g(n), A, step(n), cand(n), scale(n), diagonal(n), sg(n);
    double x_cost = 0;
    if (!P.evaluate(x.data(), &x_cost, JtJ.data(), g.data()))
    {
        sum->termination = OCHIP_RELAX_FAILURE;
        return;
    }
    for (size_t i = 0; i < n; i++)
        scale[i] = 1.0 / (1.0 + std::sqrt(JtJ[i * n + i])); // jacobi scaling, fixed from the first Jacobian
    auto gradient_max = [&]() {
        double m = 0;
        for (double e : g)
            m = std::max(m, std::abs(e));
        return m;
    };
    auto refresh_diagonal = [&]() {
        for (size_t i = 0; i < n; i++)
            diagonal[i] = std::min(std::max(JtJ[i * n + i] * scale[i] * scale[i], 1e-6), 1e32);
    };
    double x_norm = norm2(x), radius = cb::INITIAL_RADIUS, decrease_factor = 2.0, gmax = gradient_max();
    refresh_diagonal();
    sum->initial_cost = x_cost;
    sum->iterations = 1;
    int invalid = 0, iter = 0;
    auto finish = [&](int term) {
        sum->termination = term;
        sum->final_cost = x_cost;
    };
    if (gmax <= cb::GRADIENT_TOLERANCE)
        return finish(OCHIP_RELAX_CONVERGENCE_GRADIENT);
    while (true)
    {
        if (iter >= cb::MAX_ITERATIONS)
            return finish(OCHIP_RELAX_NO_CONVERGENCE);
        if (radius <= 1e-32)
            return finish(OCHIP_RELAX_CONVERGENCE_RADIUS);
        iter++;
        sum->iterations++;
        // LevenbergMarquardtStrategy::ComputeStep: (S J'J S + D'D) y = S J'r, D^2 = clamp(diag(S J'J S)) / radius
        A.assign(n * n, 0.0);
        for (size_t i = 0; i < n; i++)
        {
            for (size_t j = 0; j <= i; j++)
                A[i * n + j] = JtJ[i * n + j] * scale[i] * scale[j];
            const double d = std::sqrt(diagonal[i] / radius);
            A[i * n + i] += d * d;
            sg[i] = g[i] * scale[i];
        }
        step = sg;
        bool solved = cholesky_solve(A, step, n);
        for (double &s : step)
        {
            solved = solved && std::isfinite(s);
            s = -s;
        }
        double model_cost_change = 0;
        if (solved)
        {
            // -(step' S g + step' S J'J S step / 2)
            double lin = 0, quad = 0;
            for (size_t i = 0; i < n; i++)
            {
                lin += step[i] * sg[i];
                double row = 0;
                for (size_t j = 0; j < n; j++)
                    row += JtJ[i * n + j] * scale[i] * scale[j] * step[j];
                quad += step[i] * row;
            }
            model_cost_change = -(lin + quad / 2.0);
        }
        if (!(solved && model_cost_change > 0.0))
        {
            if (++invalid >= 5)
                return finish(OCHIP_RELAX_FAILURE);
            radius *= 0.5;
            continue;
        }
        invalid = 0;
        double step_sq = 0;
        for (size_t i = 0; i < n; i++)
        {
            cand[i] = x[i] + step[i] * scale[i];
            step_sq += (x[i] - cand[i]) * (x[i] - cand[i]);
        }
        double cand_cost = std::numeric_limits<double>::max();
        if (!P.evaluate(cand.data(), &cand_cost, nullptr, nullptr))
            cand_cost = std::numeric_limits<double>::max();
        if (std::sqrt(step_sq) <= cb::PARAMETER_TOLERANCE * (x_norm + cb::PARAMETER_TOLERANCE))
            return finish(OCHIP_RELAX_CONVERGENCE_PARAMETER);
        const double cost_change = x_cost - cand_cost;
        if (std::abs(cost_change) <= cb::FUNCTION_TOLERANCE * x_cost)
            return finish(OCHIP_RELAX_CONVERGENCE_FUNCTION);
        const double rho = cost_change / model_cost_change;
        if (rho > 1e-3)
        {
            x = cand;
            x_norm = norm2(x);
            if (!P.evaluate(x.data(), &x_cost, JtJ.data(), g.data()))
                return finish(OCHIP_RELAX_FAILURE);
            gmax = gradient_max();
            refresh_diagonal();
            const double t = 2.0 * rho - 1.0;
            radius = std::min(1e16, radius / std::max(1.0 / 3.0, 1.0 - t * t * t));
            decrease_factor = 2.0;
            sum->successful_steps++;
            if (gmax <= cb::GRADIENT_TOLERANCE)
                return finish(OCHIP_RELAX_CONVERGENCE_GRADIENT);
        }
        else
        {
            radius /= decrease_factor;
            decrease_factor *= 2.0;
            sum->unsuccessful_steps++;
        }
    }
}

// Thin SVD of the n x 3 matrix M = U diag(sigma) V' by one-sided Jacobi rotations (columns of U are made orthogonal;
// no normal equations, so sigma keeps the matrix's own conditioning).  U overwrites M.
void jacobi_svd3(std::vector<double> &M, size_t n, double sigma[3], double V[9])
{
    for (int i = 0; i < 9; i++)
        V[i] = i % 4 == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++)
    {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++)
            {
                double alpha = 0, beta = 0, gamma = 0;
                for (size_t i = 0; i < n; i++)
                {
                    alpha += M[3 * i + p] * M[3 * i + p];
                    beta += M[3 * i + q] * M[3 * i + q];
                    gamma += M[3 * i + p] * M[3 * i + q];
                }
                if (gamma == 0.0 || std::abs(gamma) <= 1e-16 * std::sqrt(alpha * beta))
                    continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::abs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (size_t i = 0; i < n; i++)
                {
                    const double up = M[3 * i + p], uq = M[3 * i + q];
                    M[3 * i + p] = c * up - s * uq;
                    M[3 * i + q] = s * up + c * uq;
                }
                for (int i = 0; i < 3; i++)
                {
                    const double vp = V[3 * i + p], vq = V[3 * i + q];
                    V[3 * i + p] = c * vp - s * vq;
                    V[3 * i + q] = s * vp + c * vq;
                }
            }
        if (!rotated)
            break;
    }
    for (int k = 0; k < 3; k++)
    {
        double s = 0;
        for (size_t i = 0; i < n; i++)
            s += M[3 * i + k] * M[3 * i + k];
        sigma[k] = std::sqrt(s);
    }
}

} // namespace

extern "C"
{

const char *och_color_balance_last_error(void)
{
    return cb_error.c_str();
}

int och_color_balance_remove_gauge(size_t n, const double *xy, double *offsets3)
{
    if (n < 3)
        return 0;
    std::vector<double> M(3 * n);
    for (size_t i = 0; i < n; i++)
        M[3 * i] = xy[2 * i], M[3 * i + 1] = xy[2 * i + 1], M[3 * i + 2] = 1.0;
    double sigma[3], V[9];
    jacobi_svd3(M, n, sigma, V);
    // the pseudo-inverse keeps the singular values above max(rows, cols) * epsilon * sigma_max
    const double smax = std::max(sigma[0], std::max(sigma[1], sigma[2]));
    const double cut = (double)std::max<size_t>(n, 3) * std::numeric_limits<double>::epsilon() * smax;
    int rank = 0;
    for (int k = 0; k < 3; k++)
        rank += sigma[k] > cut;
    for (int c = 0; c < 3; c++)
    {
        double plane[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++)
        {
            if (!(sigma[k] > cut))
                continue;
            double ub = 0; // (u_k . b) / sigma_k with u_k = M_k / sigma_k
            for (size_t i = 0; i < n; i++)
                ub += M[3 * i + k] * offsets3[3 * i + c];
            ub /= sigma[k] * sigma[k];
            for (int i = 0; i < 3; i++)
                plane[i] += V[3 * i + k] * ub;
        }
        for (size_t i = 0; i < n; i++)
        {
            const double fitted = plane[0] * xy[2 * i] + plane[1] * xy[2 * i + 1] + plane[2];
            offsets3[3 * i + c] -= fitted;
        }
    }
    return rank;
}

int och_color_balance_evaluate(ochip_ctx *ctx, const ochip_color_corr *corr, size_t n_corr, size_t n_cams, const uint64_t *cam_ids,
                               const double *color6, size_t n_models, const uint32_t *model_ids, const double *vig3, double *cost,
                               double *JtJ, double *Jtr, int32_t *cam_col, int32_t *model_col)
{
    cb_error.clear();
    if (!corr || !n_corr || !cam_ids || !model_ids || !color6 || !vig3 || !cost || (JtJ != nullptr) != (Jtr != nullptr))
        return cb_error = "och_color_balance_evaluate: bad argument", -1;
    if (ctx)
    {
        int32_t n_dev = 0;
        const int rc = ochip_color_balance_evaluate(ctx, corr, n_corr, cam_ids, (uint32_t)n_cams, model_ids, (uint32_t)n_models,
                                                    color6, vig3, cost, &n_dev, JtJ, Jtr, cam_col, model_col);
        if (rc < 0)
            return cb_error = std::string("ochip_color_balance_evaluate: ") + ochip_last_error(ctx), -1;
        return rc;
    }
    tables t;
    if (!build_tables(corr, n_corr, cam_ids, n_cams, model_ids, n_models, &t))
        return -1;
    problem P(corr, n_corr, &t);
    if (JtJ && P.n > CPU_MAX_UNKNOWNS)
        return cb_error = "the CPU route holds at most " + std::to_string(CPU_MAX_UNKNOWNS) + " unknowns", -1;
    std::vector<double> x(P.n);
    std::memcpy(x.data(), color6, sizeof(double) * cb::CAM_UNKNOWNS * n_cams);
    std::memcpy(x.data() + cb::CAM_UNKNOWNS * n_cams, vig3, sizeof(double) * cb::MODEL_UNKNOWNS * n_models);
    for (size_t i = 0; cam_col && i < n_cams; i++)
        cam_col[i] = (int32_t)(cb::CAM_UNKNOWNS * i);
    for (size_t m = 0; model_col && m < n_models; m++)
        model_col[m] = (int32_t)(cb::CAM_UNKNOWNS * n_cams + cb::MODEL_UNKNOWNS * m);
    return P.evaluate(x.data(), cost, JtJ, Jtr) ? 0 : 1;
}

int och_color_balance_evaluate_plan(const ochip_color_corr *corr, size_t n_corr, size_t n_cams, const uint64_t *cam_ids,
                                    const double *color6, size_t n_models, const uint32_t *model_ids, const double *vig3, double *cost,
                                    double *JtJ, double *Jtr, int32_t *cam_col, int32_t *model_col, int32_t *layout4)
{
    cb_error.clear();
    if (!color6 || !vig3 || !cost || (JtJ != nullptr) != (Jtr != nullptr))
        return cb_error = "och_color_balance_evaluate_plan: bad argument", -1;
    cb::plan P;
    if (!cb::build_plan(corr, n_corr, cam_ids, (uint32_t)n_cams, model_ids, (uint32_t)n_models, &P, &cb_error))
        return -1;
    if (JtJ && (size_t)P.n > CPU_MAX_UNKNOWNS)
        return cb_error = "the host evaluation holds at most " + std::to_string(CPU_MAX_UNKNOWNS) + " unknowns", -1;
    std::vector<double> x((size_t)P.n, 0.0);
    for (size_t i = 0; i < n_cams; i++)
    {
        std::memcpy(&x[P.cam_t[i]], color6 + cb::CAM_UNKNOWNS * i, sizeof(double) * cb::CAM_UNKNOWNS);
        if (cam_col)
            cam_col[i] = P.cam_t[i];
    }
    for (size_t m = 0; m < n_models; m++)
    {
        std::memcpy(&x[P.model_t[m]], vig3 + cb::MODEL_UNKNOWNS * m, sizeof(double) * cb::MODEL_UNKNOWNS);
        if (model_col)
            model_col[m] = P.model_t[m];
    }
    if (layout4)
    {
        layout4[0] = P.tail_begin, layout4[1] = (int32_t)std::max<size_t>(P.region_begin.size(), 1), layout4[2] = P.n_separators;
        layout4[3] = (int32_t)P.chunks.size();
    }
    return cb::plan_evaluate_host(P, x.data(), cost, JtJ, Jtr) ? 0 : 1;
}

int och_color_balance_solve(const och_graph *g, ochip_ctx *ctx, const ochip_color_corr *corr, size_t n_corr, size_t n_positions,
                            const uint64_t *position_ids, const double *position_xy, size_t cam_capacity, uint64_t *cam_ids_out,
                            double *color6_out, size_t *n_cams_out, size_t model_capacity, uint32_t *model_ids_out,
                            double *vig3_out, size_t *n_models_out, double *summary4)
{
    cb_error.clear();
    if (!n_cams_out || !n_models_out || !summary4 || (n_corr && !corr) || (n_positions && (!position_ids || !position_xy)))
        return cb_error = "och_color_balance_solve: bad argument", -1;
    *n_cams_out = *n_models_out = 0;
    summary4[0] = summary4[1] = summary4[2] = 0;
    summary4[3] = OCHIP_RELAX_FAILURE;
    if (n_corr == 0) // solveColorBalance: "no correspondences to solve", success = false, empty tables
        return 0;
    tables t;
    if (!build_tables(corr, n_corr, nullptr, 0, nullptr, 0, &t))
        return -1;
    const size_t nc = t.cam_ids.size(), nm = t.model_ids.size();
    *n_cams_out = nc, *n_models_out = nm;
    if (nc > cam_capacity || nm > model_capacity || !cam_ids_out || !color6_out || !model_ids_out || !vig3_out)
        return cb_error = "och_color_balance_solve: the output tables are too small", -1;
    ochip_relax_summary sum{};
    std::vector<double> x(cb::CAM_UNKNOWNS * nc + cb::MODEL_UNKNOWNS * nm, 0.0);
    if (ctx)
    {
        const int rc = ochip_color_balance_solve(ctx, corr, n_corr, t.cam_ids.data(), (uint32_t)nc, t.model_ids.data(), (uint32_t)nm,
                                                 x.data(), x.data() + cb::CAM_UNKNOWNS * nc, &sum);
        if (rc != OCHIP_OK)
            return cb_error = std::string("ochip_color_balance_solve: ") + ochip_last_error(ctx), -1;
    }
    else
    {
        if (x.size() > CPU_MAX_UNKNOWNS)
            return cb_error = "the CPU route holds at most " + std::to_string(CPU_MAX_UNKNOWNS) + " unknowns (" +
                              std::to_string(x.size()) + " asked): use the device route",
                   -1;
        problem P(corr, n_corr, &t);
        solve_cpu(P, x, &sum);
    }
    // Gauge: the plane a x + b y + c fitted to the positioned cameras' offsets, per Lab channel, is subtracted from them
    {
        std::vector<std::pair<uint64_t, size_t>> explicit_pos(n_positions);
        for (size_t i = 0; i < n_positions; i++)
            explicit_pos[i] = {position_ids[i], i};
        std::sort(explicit_pos.begin(), explicit_pos.end());
        std::vector<size_t> rows;
        std::vector<double> xy, off;
        for (size_t i = 0; i < nc; i++)
        {
            double px = 0, py = 0;
            bool have = false;
            const auto it = std::lower_bound(explicit_pos.begin(), explicit_pos.end(), std::make_pair(t.cam_ids[i], (size_t)0));
            if (it != explicit_pos.end() && it->first == t.cam_ids[i])
                px = position_xy[2 * it->second], py = position_xy[2 * it->second + 1], have = true;
            else if (g)
                if (const auto *node = g->graph.getNode(t.cam_ids[i]))
                    px = node->payload.position[0], py = node->payload.position[1], have = true;
            if (!have)
                continue;
            rows.push_back(i);
            xy.push_back(px), xy.push_back(py);
            for (int c = 0; c < 3; c++)
                off.push_back(x[cb::CAM_UNKNOWNS * i + c]);
        }
        och_color_balance_remove_gauge(rows.size(), xy.data(), off.data());
        if (rows.size() >= 3)
            for (size_t k = 0; k < rows.size(); k++)
                for (int c = 0; c < 3; c++)
                    x[cb::CAM_UNKNOWNS * rows[k] + c] = off[3 * k + c];
    }
    std::memcpy(cam_ids_out, t.cam_ids.data(), sizeof(uint64_t) * nc);
    std::memcpy(model_ids_out, t.model_ids.data(), sizeof(uint32_t) * nm);
    std::memcpy(color6_out, x.data(), sizeof(double) * cb::CAM_UNKNOWNS * nc);
    std::memcpy(vig3_out, x.data() + cb::CAM_UNKNOWNS * nc, sizeof(double) * cb::MODEL_UNKNOWNS * nm);
    summary4[0] = sum.termination != OCHIP_RELAX_FAILURE; // CONVERGENCE or NO_CONVERGENCE
    summary4[1] = sum.final_cost;
    summary4[2] = sum.iterations;
    summary4[3] = sum.termination;
    return 0;
}

} // extern "C"
