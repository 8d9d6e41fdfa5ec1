// Colour balance (src/ortho/color_balance.cpp, include/opencalibration/ortho/radiometric_cost.hpp): the arithmetic of one
// colour correspondence, shared by the device engine (color_balance.hip) and the CPU route (host/color_balance.cpp).
// Both are compiled with -ffp-contract=off: an expression written here rounds the same way on either side.
//
// One correspondence is one residual block of three residuals under HuberLoss(5) with Ceres' corrector
// (RadiometricMatchCost and RadiometricMatchCostSharedVig are one formula: with equal model ids the two vignetting terms
// act on the same three unknowns, and their derivatives add):
//     r_c = (obs_a[c] - off_a[c]) - (obs_b[c] - off_b[c]),
//     c == 0: each side also loses (vig . (r^2, r^4, r^6) + brdf * theta^2) + slope . (nx, ny)
// r^2 and theta^2 are FLOAT products widened to double, r^4 and r^6 are formed in double from r^2, nx and ny are
// widened floats - as the functor's T(_r_a * _r_a) and T(_nx_a) do.
//
// A block's columns are numbered locally: 0..5 the pair's first camera (lab_offset 3, brdf, slope 2), 6..11 its second
// camera, 12..14 the vignetting of the first camera's model, 15..17 that of the second camera's model.  The pair's
// first camera is the one that comes first in the solve's camera table; `flip` says that the correspondence's `a` is
// the second one.  With a shared model the columns 15..17 stay zero and 12..14 carry both sides.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define OCHIP_CB_HD __host__ __device__ inline
#else
#define OCHIP_CB_HD inline
#endif

namespace ochip_cb
{

constexpr int CAM_UNKNOWNS = 6;   // lab_offset[3], brdf, slope[2]
constexpr int MODEL_UNKNOWNS = 3; // vignetting coefficients
constexpr int BLOCK_COLS = 18;    // local columns of one correspondence
constexpr int BLOCK_TRI = BLOCK_COLS * (BLOCK_COLS + 1) / 2;
constexpr double HUBER_A = 5.0;         // ceres::HuberLoss(5.0), color_balance.cpp:76
constexpr double PRIOR_WEIGHT = 0.1;    // times sqrt(max(1, count)), color_balance.cpp:104-138
// ceres::Solver::Options of solveColorBalance (color_balance.cpp:140-148); the rest are Ceres' defaults
constexpr int MAX_ITERATIONS = 20;
constexpr double FUNCTION_TOLERANCE = 1e-4, GRADIENT_TOLERANCE = 1e-6, PARAMETER_TOLERANCE = 1e-4;
constexpr double INITIAL_RADIUS = 1e4;

// the fields of a ColorCorrespondence the functor reads; side 0 = a, 1 = b
struct obs
{
    float lab[2][3];
    float radius[2], angle[2], nx[2], ny[2];
};

OCHIP_CB_HD int tri_index(int i, int j) // packed lower triangle, i >= j
{
    return i * (i + 1) / 2 + j;
}

OCHIP_CB_HD double prior_weight(uint64_t count)
{
    return PRIOR_WEIGHT * sqrt((double)(count > 1 ? count : 1));
}

// Residuals, cost and (J != nullptr) the Jacobian of one correspondence, loss applied: res[3] and J[3][18] are what
// Ceres hands to the linear solver (corrector.cc), *cost = rho(|r|^2) / 2.  cam[side], vig[side]: the parameters of the
// correspondence's a / b side (vig[0] == vig[1] values for a shared model).  Returns false when a residual is not finite.
OCHIP_CB_HD bool eval_block(const obs &o, const double *const cam[2], const double *const vig[2], bool shared, bool flip,
                            double *res, double *J, double *cost)
{
    double corr[2][3], d_vig[2][3], d_brdf[2];
    for (int s = 0; s < 2; s++)
    {
        const double r2 = (double)(o.radius[s] * o.radius[s]);
        const double vig_corr = vig[s][0] * r2 + vig[s][1] * r2 * r2 + vig[s][2] * r2 * r2 * r2;
        const double th2 = (double)(o.angle[s] * o.angle[s]);
        const double brdf_corr = cam[s][3] * th2;
        const double slope_corr = cam[s][4] * (double)o.nx[s] + cam[s][5] * (double)o.ny[s];
        for (int c = 0; c < 3; c++)
            corr[s][c] = (double)o.lab[s][c] - cam[s][c];
        corr[s][0] -= vig_corr + brdf_corr + slope_corr;
        d_vig[s][0] = r2, d_vig[s][1] = r2 * r2, d_vig[s][2] = r2 * r2 * r2;
        d_brdf[s] = th2;
    }
    double sq = 0;
    bool finite = true;
    for (int c = 0; c < 3; c++)
    {
        res[c] = corr[0][c] - corr[1][c];
        finite = finite && std::isfinite(res[c]);
        sq += res[c] * res[c];
    }
    // HuberLoss::Evaluate
    double rho0 = sq, rho1 = 1.0, rho2 = 0.0;
    if (sq > HUBER_A * HUBER_A)
    {
        const double r = sqrt(sq);
        rho0 = 2.0 * HUBER_A * r - HUBER_A * HUBER_A;
        rho1 = HUBER_A / r;
        if (rho1 < 2.2250738585072014e-308)
            rho1 = 2.2250738585072014e-308;
        rho2 = -rho1 / (2.0 * sq);
    }
    *cost = 0.5 * rho0;
    // Corrector::Corrector
    const double sqrt_rho1 = sqrt(rho1);
    double residual_scaling = sqrt_rho1, alpha_sq_norm = 0.0;
    if (!(sq == 0.0 || rho2 <= 0.0))
    {
        const double D = 1.0 + 2.0 * sq * rho2 / rho1;
        const double alpha = 1.0 - sqrt(D);
        residual_scaling = sqrt_rho1 / (1.0 - alpha);
        alpha_sq_norm = alpha / sq;
    }
    if (J)
    {
        for (int k = 0; k < 3 * BLOCK_COLS; k++)
            J[k] = 0.0;
        for (int s = 0; s < 2; s++)
        {
            const double sign = s == 0 ? -1.0 : 1.0; // d r / d (side a's parameters) = -(d corr_a's subtrahend)
            const int cb = (s == 0) != flip ? 0 : CAM_UNKNOWNS;
            const int vb = shared ? 12 : ((s == 0) != flip ? 12 : 15);
            for (int c = 0; c < 3; c++)
                J[c * BLOCK_COLS + cb + c] = sign;
            J[cb + 3] = sign * d_brdf[s];
            J[cb + 4] = sign * (double)o.nx[s];
            J[cb + 5] = sign * (double)o.ny[s];
            for (int k = 0; k < 3; k++)
                J[vb + k] += sign * d_vig[s][k];
        }
        // Corrector::CorrectJacobian
        for (int k = 0; k < BLOCK_COLS; k++)
        {
            double *c0 = J + k, *c1 = J + BLOCK_COLS + k, *c2 = J + 2 * BLOCK_COLS + k;
            if (alpha_sq_norm == 0.0)
            {
                *c0 *= sqrt_rho1, *c1 *= sqrt_rho1, *c2 *= sqrt_rho1;
                continue;
            }
            const double rtj = *c0 * res[0] + *c1 * res[1] + *c2 * res[2];
            *c0 = sqrt_rho1 * (*c0 - alpha_sq_norm * res[0] * rtj);
            *c1 = sqrt_rho1 * (*c1 - alpha_sq_norm * res[1] * rtj);
            *c2 = sqrt_rho1 * (*c2 - alpha_sq_norm * res[2] * rtj);
        }
    }
    for (int c = 0; c < 3; c++)
        res[c] *= residual_scaling;
    return finite;
}

// One entry of a block's J'J (i >= j) and J'r from the corrected Jacobian and residuals
OCHIP_CB_HD double jtj_entry(const double *J, int i, int j)
{
    return J[i] * J[j] + J[BLOCK_COLS + i] * J[BLOCK_COLS + j] + J[2 * BLOCK_COLS + i] * J[2 * BLOCK_COLS + j];
}
OCHIP_CB_HD double jtr_entry(const double *J, const double *res, int i)
{
    return J[i] * res[0] + J[BLOCK_COLS + i] * res[1] + J[2 * BLOCK_COLS + i] * res[2];
}

} // namespace ochip_cb
