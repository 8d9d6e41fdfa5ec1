// The rules of one Levenberg-Marquardt step that every user of the relax solve shares, once: the host trust-region loop
// (relax_lm.hip: lm_solve), the three engines (relax.hip, relax_general.hip, relax_points.hip) and the resident bootstrap
// chain (relax_chain.hip), which must run the same solves and the same iterations as the host loop to the bit
// (tests/test_gpu_bootstrap_chain.py).  Host loops and gfx950 kernels both run these; a plain C++17 compiler can include
// the header (tests/lm_rules_driver.cpp).  Ceres semantics throughout: TrustRegionMinimizer, LevenbergMarquardtStrategy,
// EigenQuaternionManifold.
#pragma once

#include "../../include/ochip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OCHIP_LM_HD __host__ __device__ __forceinline__
#else
#define OCHIP_LM_HD inline
#endif

namespace ochip
{

// the ceres::Solver::Options of RelaxProblem (relax_problem.cpp:30-37): 100 iterations, radius 1, function / gradient /
// parameter tolerances
OCHIP_LM_HD ochip_relax_options lm_reference_options()
{
    return ochip_relax_options{100, 1.0, 1e-6, 1e-10, 1e-8};
}

// o = exp(d) * q (x, y, z, w): the Plus of the orientation's manifold.  A zero step copies q.
OCHIP_LM_HD void lm_quat_plus(const double q[4], const double d[3], double o[4])
{
    const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (nrm == 0.0)
    {
        for (int k = 0; k < 4; k++)
            o[k] = q[k];
    }
    else
    {
        const double s = sin(nrm) / nrm;
        const double dx = s * d[0], dy = s * d[1], dz = s * d[2], dw = cos(nrm);
        const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
        o[3] = dw * qw - dx * qx - dy * qy - dz * qz;
        o[0] = dw * qx + dx * qw + dy * qz - dz * qy;
        o[1] = dw * qy + dy * qw + dz * qx - dx * qz;
        o[2] = dw * qz + dz * qw + dx * qy - dy * qx;
    }
}

// orientation.normalize() after a solve (relax_problem.cpp:1410-1413), Eigen's rule: a quaternion of squared norm exactly
// 0 is left alone (and so is one whose squared norm is NaN: the test fails for it, as Eigen's does)
OCHIP_LM_HD void lm_quat_normalize(double q[4])
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n2 > 0.0)
    {
        const double n = sqrt(n2);
        for (int k = 0; k < 4; k++)
            q[k] = q[k] / n;
    }
}

// jacobi scaling of a column from the diagonal of the solve's first J'J
OCHIP_LM_HD double lm_jacobi_scale(double d)
{
    return 1.0 / (1.0 + sqrt(d));
}
// the damping's diagonal, v = diag(J'J) scale^2: std::min(std::max(v, 1e-6), 1e32) as comparisons - NaN passes through
OCHIP_LM_HD double lm_clamp_diagonal(double v)
{
    const double lo = v < 1e-6 ? 1e-6 : v;
    return 1e32 < lo ? 1e32 : lo;
}
// D_ii^2 = diagonal_i / radius as LevenbergMarquardtStrategy forms it: the square root, then squared
OCHIP_LM_HD double lm_damping(double diagonal, double radius)
{
    const double dd = sqrt(diagonal / radius);
    return dd * dd;
}

// The trust region of a solve.  Every expression is lm_solve's (std::max / std::min spelled as the comparisons they are:
// a NaN in 1 - (2 rho - 1)^3 gives 1/3, a NaN radius gives 1e16).
struct lm_trust
{
    double radius, decrease;
    int invalid;

    OCHIP_LM_HD void start(double initial_radius)
    {
        radius = initial_radius;
        decrease = 2.0;
        invalid = 0;
    }
    OCHIP_LM_HD static bool step_is_valid(int chol_fail, double model_cost_change)
    {
        return !chol_fail && std::isfinite(model_cost_change) && model_cost_change > 0.0;
    }
    // an invalid step: true = the fifth in a row, the solve fails; else the radius is halved
    OCHIP_LM_HD bool on_invalid()
    {
        if (++invalid >= 5)
            return true;
        radius *= 0.5;
        return false;
    }
    OCHIP_LM_HD void on_valid()
    {
        invalid = 0;
    }
    OCHIP_LM_HD static bool parameter_converged(double step_norm, double x_norm, double tol)
    {
        return step_norm <= tol * (x_norm + tol);
    }
    OCHIP_LM_HD static bool function_converged(double cost_change, double x_cost, double tol)
    {
        return fabs(cost_change) <= tol * x_cost;
    }
    OCHIP_LM_HD static bool accepts(double rho)
    {
        return rho > 1e-3;
    }
    OCHIP_LM_HD void on_accept(double rho)
    {
        const double t = 2.0 * rho - 1.0;
        const double b = 1.0 - t * t * t;
        radius = radius / (1.0 / 3.0 < b ? b : 1.0 / 3.0);
        radius = radius < 1e16 ? radius : 1e16;
        decrease = 2.0;
    }
    OCHIP_LM_HD void on_reject()
    {
        radius = radius / decrease;
        decrease *= 2.0;
    }
    OCHIP_LM_HD bool radius_exhausted() const
    {
        return radius <= 1e-32;
    }
};

#if defined(__HIPCC__)
// Sum / maximum of one value per thread over a workgroup of TG threads, by the halving tree (a fixed order: the bits do not
// depend on who calls).  sh: TG doubles of LDS.  Every thread gets the result.  The barriers are the tree's own: a caller
// whose threads may still read sh from before puts a barrier in front, one that writes sh again puts one behind.
template <int TG> __device__ __forceinline__ double lm_block_sum(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = TG / 2; s > 0; s >>= 1)
    {
        if (t < s)
            sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}
template <int TG> __device__ __forceinline__ double lm_block_max(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = TG / 2; s > 0; s >>= 1)
    {
        if (t < s)
            sh[t] = fmax(sh[t], sh[t + s]);
        __syncthreads();
    }
    return sh[0];
}

// The cameras of a candidate step, by the TG threads of one workgroup: o = q (+) d with d = alpha * (-y * scale) at the
// camera's tangent offset cam_t[c]; a camera without unknowns (cam_t < 0) is copied.  Adds this thread's share of
// |q - o|^2 to *sn and of |o|^2 to *xn, over the cameras with unknowns.
template <int TG>
__device__ __forceinline__ void lm_candidate_cams(uint32_t n_cams, const int32_t *cam_t, const double *Q, double *O, const double *y,
                                                  const double *scale, double alpha, double *sn, double *xn)
{
    for (uint32_t c = threadIdx.x; c < n_cams; c += TG)
    {
        const int tc = cam_t[c];
        const double *q = Q + (size_t)c * 4;
        double *o = O + (size_t)c * 4;
        if (tc < 0)
        {
            for (int k = 0; k < 4; k++)
                o[k] = q[k];
            continue;
        }
        double d[3];
        for (int k = 0; k < 3; k++)
            d[k] = alpha * (-y[tc + k] * scale[tc + k]);
        lm_quat_plus(q, d, o);
        for (int k = 0; k < 4; k++)
        {
            *sn += (q[k] - o[k]) * (q[k] - o[k]);
            *xn += o[k] * o[k];
        }
    }
}
#endif

} // namespace ochip
