// ORACLE — test infrastructure only (see oracle.hpp).
//
// One evaluation and one Levenberg-Marquardt step of the points engine's problem (the flat ochip_relaxp_desc the device
// takes) the way the reference's Problem and Ceres' LevenbergMarquardtStrategy treat it, on the FULL system - nothing is
// eliminated: every observation through the restated PixelErrorCost_* functors on Jets of a selectable scalar (double, or
// long double for a reference with 11 more bits), the EigenQuaternionManifold / SubsetManifold plus-Jacobians,
// HuberLoss(huber_a) with the Triggs corrector, DistortionMonotonicityCost, then J'J, J'r and the cost summed in that
// scalar.  tests/test_relaxp_eval_oracle.py checks it against its own central differences;
// tests/test_gpu_relaxp_eval.py compares the device's evaluation and Schur step (ochip_relaxp_evaluate / _step) with it.
//
// Residual blocks (the row order of J): observation 2p (camera grp_cam[2g], 2 rows), observation 2p + 1 (camera
// grp_cam[2g + 1]) of every point p in index order; then the 10 rows of DistortionMonotonicityCost when functor >= 2 and
// mono_observations > 0.  Canonical column order: 3 per variable camera in index order, then f, ppx ppy, the free
// k's, p1 p2 (the n REDUCED unknowns), then 3 per point.  A camera is variable when it is optimised, not
// structure_only, and observes a point; the lens parameters the functor level exposes are variable when they are
// optimised, not structure_only, and there is a point.
#include "../include/ochip.h"
#include "mini_ceres.hpp"
#include "relax_functors.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace oracle
{
namespace
{

// perturbations of the reference, for the tests that show the bounds bite
enum
{
    PMUT_NONE = 0,
    PMUT_PARTIAL = 1,         // block `arg`: its largest corrected partial times (1 + 1e-9)
    PMUT_NO_CORR_J = 2,       // the corrector applied to the residuals but not to the Jacobian
    PMUT_DROP_SCHUR = 3,      // step: point `arg` left out of the Schur term and the reduced right-hand side
    PMUT_NO_POINT_DAMPING = 4 // step: D^2 left off the point columns
};

template <typename S> struct PEval
{
    const ochip_relaxp_desc &d;
    bool structure_only;
    int raw = 0, mutate = PMUT_NONE, mutate_arg = -1;
    std::vector<S> q, X, m;
    std::vector<int> cam_t;
    int lens_t[8];
    int nk = 0, n = 0, N = 0;
    bool mono = false;
    std::vector<uint32_t> pt_group;
    // outputs (rows x N, row-major)
    std::vector<S> J, r, JtJ, Jtr;
    std::vector<int32_t> row_blk;
    std::vector<uint8_t> touch;
    S cost = 0;
    bool failed = false;

    PEval(const ochip_relaxp_desc &d_, bool so) : d(d_), structure_only(so)
    {
        q.assign(d.cam_q, d.cam_q + 4 * (size_t)d.n_cams);
        X.assign(d.point_xyz, d.point_xyz + 3 * (size_t)d.n_points);
        m.assign(d.model, d.model + 8);
        nk = std::min<int>(d.n_radial_free, 3);
        mono = d.functor >= 2 && d.mono_observations > 0;
        pt_group.assign(d.n_points, 0);
        std::vector<char> used(d.n_cams, 0);
        for (uint32_t g = 0; g < d.n_groups; g++)
            for (uint32_t p = d.grp_first[g]; p < d.grp_first[g + 1]; p++)
            {
                pt_group[p] = g;
                used[d.grp_cam[2 * g]] = used[d.grp_cam[2 * g + 1]] = 1;
            }
        cam_t.assign(d.n_cams, -1);
        for (uint32_t c = 0; c < d.n_cams; c++)
            if (d.cam_optimize[c] && used[c] && !structure_only)
                cam_t[c] = n, n += 3;
        for (int k = 0; k < 8; k++)
            lens_t[k] = -1;
        if (!structure_only && d.n_points > 0)
        {
            if (d.functor >= 1 && d.opt_focal)
                lens_t[0] = n++;
            if (d.functor >= 1 && d.opt_principal)
                lens_t[1] = n++, lens_t[2] = n++;
            if (d.functor >= 2)
                for (int k = 0; k < nk; k++)
                    lens_t[3 + k] = n++;
            if (d.functor >= 3)
                lens_t[6] = n++, lens_t[7] = n++;
        }
        N = n + 3 * (int)d.n_points;
    }
    int point_t(uint32_t p) const
    {
        return n + 3 * (int)p;
    }
    // the lens parameter blocks (focal 1, principal point 2, radial 3, tangential 2) and whether one is variable
    static constexpr int blk_first[4] = {0, 1, 3, 6}, blk_size[4] = {1, 2, 3, 2};
    bool lens_block_variable(int b) const
    {
        for (int k = 0; k < blk_size[b]; k++)
            if (lens_t[blk_first[b] + k] >= 0)
                return true;
        return false;
    }
    // x <- x [+] delta over the canonical columns
    void plus(const S *delta)
    {
        for (uint32_t c = 0; c < d.n_cams; c++)
            if (cam_t[c] >= 0)
            {
                S out[4];
                mc::quat_plus_t<S>(&q[4 * c], delta + cam_t[c], out);
                for (int k = 0; k < 4; k++)
                    q[4 * c + k] = out[k];
            }
        for (int k = 0; k < 8; k++)
            if (lens_t[k] >= 0)
                m[k] += delta[lens_t[k]];
        for (size_t i = 0; i < X.size(); i++)
            X[i] += delta[n + i];
    }

    // the loss, the corrector and the assembly of one block whose residuals out[0 .. nr) and tangent rows Jb (nr x N) are given
    void finish_block(int b, int nr, const S *res, std::vector<S> &Jb, const std::vector<uint8_t> &tb, bool with_loss, bool ok)
    {
        const int row0 = (int)r.size();
        S sq = 0;
        for (int i = 0; i < nr; i++)
        {
            r.push_back(res[i]);
            row_blk.push_back(b);
            sq += res[i] * res[i];
            ok &= std::isfinite(res[i]);
        }
        for (S v : Jb)
            ok &= std::isfinite(v);
        failed |= !ok;
        S rho[3] = {sq, S(1), S(0)};
        if (with_loss && !raw)
            mc::huber_rho<S>(S(d.huber_a), S(d.huber_a) * S(d.huber_a), sq, rho);
        cost += S(0.5) * rho[0];
        if (with_loss && !raw)
        {
            S sqrt_rho1, scaling, alpha_sq_norm;
            mc::corrector_terms<S>(sq, rho, &sqrt_rho1, &scaling, &alpha_sq_norm);
            if (mutate != PMUT_NO_CORR_J)
                for (int c = 0; c < N; c++)
                {
                    bool any = false;
                    for (int i = 0; i < nr; i++)
                        any |= Jb[(size_t)i * N + c] != S(0);
                    if (!any)
                        continue;
                    S rtj = 0;
                    for (int i = 0; i < nr; i++)
                        rtj += Jb[(size_t)i * N + c] * r[row0 + i];
                    for (int i = 0; i < nr; i++)
                        Jb[(size_t)i * N + c] = sqrt_rho1 * (Jb[(size_t)i * N + c] - alpha_sq_norm * r[row0 + i] * rtj);
                }
            for (int i = 0; i < nr; i++)
                r[row0 + i] *= scaling;
        }
        if (mutate == PMUT_PARTIAL && b == mutate_arg)
        {
            size_t at = 0;
            for (size_t e = 0; e < Jb.size(); e++)
                if (std::abs(Jb[e]) > std::abs(Jb[at]))
                    at = e;
            Jb[at] *= S(1) + S(1e-9);
        }
        J.insert(J.end(), Jb.begin(), Jb.end());
        touch.insert(touch.end(), tb.begin(), tb.end());
        std::vector<int> nz;
        for (int i = 0; i < nr; i++)
        {
            const S *row = &Jb[(size_t)i * N];
            nz.clear();
            for (int a = 0; a < N; a++)
                if (row[a] != S(0))
                    nz.push_back(a);
            for (int a : nz)
            {
                Jtr[a] += row[a] * r[row0 + i];
                for (int c : nz)
                    JtJ[(size_t)a * N + c] += row[a] * row[c];
            }
        }
    }

    void observation(uint32_t o)
    {
        using J_t = Jet<15, S>; // quaternion 4 | point 3 | f | pp 2 | radial 3 | tangential 2
        const uint32_t p = o >> 1, g = pt_group[p], c = d.grp_cam[2 * g + (o & 1)];
        J_t x[15];
        for (int k = 0; k < 4; k++)
            x[k] = J_t(q[4 * (size_t)c + k], k);
        for (int k = 0; k < 3; k++)
            x[4 + k] = J_t(X[3 * (size_t)p + k], 4 + k);
        for (int k = 0; k < 8; k++)
            x[7 + k] = J_t(m[k], 7 + k);
        J_t out[2];
        bool ok;
        auto fill = [&](PixelErrorCost &f) {
            f.loc = {d.cam_pos[3 * (size_t)c], d.cam_pos[3 * (size_t)c + 1], d.cam_pos[3 * (size_t)c + 2]};
            f.model.focal_length_pixels = d.model[0];
            f.model.principle_point[0] = d.model[1], f.model.principle_point[1] = d.model[2];
            for (int k = 0; k < 3; k++)
                f.model.radial_distortion[k] = d.model[3 + k];
            f.model.tangential_distortion[0] = d.model[6], f.model.tangential_distortion[1] = d.model[7];
            f.pixel[0] = d.obs_px[2 * (size_t)o], f.pixel[1] = d.obs_px[2 * (size_t)o + 1];
        };
        switch (d.functor)
        {
        case 0: {
            PixelErrorCost_Orientation f;
            fill(f);
            ok = f(x, x + 4, out);
            break;
        }
        case 1: {
            PixelErrorCost_OrientationFocal f;
            fill(f);
            ok = f(x, x + 4, x + 7, x + 8, out);
            break;
        }
        case 2: {
            PixelErrorCost_OrientationFocalRadial f;
            fill(f);
            ok = f(x, x + 4, x + 7, x + 8, x + 10, out);
            break;
        }
        default: {
            PixelErrorCost_OrientationFocalRadialTangential f;
            fill(f);
            ok = f(x, x + 4, x + 7, x + 8, x + 10, x + 13, out);
            break;
        }
        }
        std::vector<S> Jb((size_t)2 * N, S(0));
        std::vector<uint8_t> tb((size_t)2 * N, 0);
        S res[2];
        for (int i = 0; i < 2; i++)
        {
            res[i] = out[i].a;
            if (cam_t[c] >= 0)
            {
                S PJ[12];
                mc::quat_plus_jacobian_t<S>(&q[4 * (size_t)c], PJ);
                for (int col = 0; col < 3; col++)
                {
                    S v = 0;
                    for (int k = 0; k < 4; k++)
                        v += out[i].v[k] * PJ[k * 3 + col];
                    Jb[(size_t)i * N + cam_t[c] + col] = v;
                    tb[(size_t)i * N + cam_t[c] + col] = 1;
                }
            }
            // (a level the functor does not expose, or a constant coordinate of the SubsetManifold, has lens_t < 0)
            for (int k = 0; k < 8; k++)
                if (lens_t[k] >= 0)
                {
                    Jb[(size_t)i * N + lens_t[k]] = out[i].v[7 + k];
                    tb[(size_t)i * N + lens_t[k]] = 1;
                }
            for (int k = 0; k < 3; k++)
            {
                Jb[(size_t)i * N + point_t(p) + k] = out[i].v[4 + k];
                tb[(size_t)i * N + point_t(p) + k] = 1;
            }
        }
        finish_block((int)o, 2, res, Jb, tb, true, ok);
    }

    void monotonicity()
    {
        using J_t = Jet<3, S>;
        DistortionMonotonicityCost f;
        f.r_max = d.mono_r_max;
        f.weight = std::sqrt(d.mono_observations / 10.0);
        J_t x[3], out[10];
        for (int k = 0; k < 3; k++)
            x[k] = J_t(m[3 + k], k);
        const bool ok = f(x, out);
        std::vector<S> Jb((size_t)10 * N, S(0));
        std::vector<uint8_t> tb((size_t)10 * N, 0);
        S res[10];
        for (int i = 0; i < 10; i++)
        {
            res[i] = out[i].a;
            for (int k = 0; k < 3; k++)
                if (lens_t[3 + k] >= 0)
                {
                    Jb[(size_t)i * N + lens_t[3 + k]] = out[i].v[k];
                    tb[(size_t)i * N + lens_t[3 + k]] = 1;
                }
        }
        finish_block(2 * (int)d.n_points, 10, res, Jb, tb, false, ok);
    }

    void run()
    {
        J.clear(), r.clear(), row_blk.clear(), touch.clear();
        JtJ.assign((size_t)N * N, S(0));
        Jtr.assign(N, S(0));
        cost = 0;
        failed = false;
        for (uint32_t o = 0; o < 2 * d.n_points; o++)
            observation(o);
        if (mono)
            monotonicity();
    }
};

template <typename S> void to_double(const std::vector<S> &v, double *out)
{
    if (out)
        for (size_t i = 0; i < v.size(); i++)
            out[i] = (double)v[i];
}

// in-place dense Cholesky solve A x = b of the lower triangle of A (k x k, row-major), nrhs right-hand sides (k x nrhs)
template <typename S> bool chol_solve(std::vector<S> &A, int k, S *b, int nrhs)
{
    using std::sqrt;
    for (int j = 0; j < k; j++)
    {
        S dj = A[(size_t)j * k + j];
        for (int t = 0; t < j; t++)
            dj -= A[(size_t)j * k + t] * A[(size_t)j * k + t];
        if (!(dj > S(0)) || !std::isfinite(dj))
            return false;
        const S l = sqrt(dj);
        A[(size_t)j * k + j] = l;
        for (int i = j + 1; i < k; i++)
        {
            S v = A[(size_t)i * k + j];
            const S *ri = &A[(size_t)i * k], *rj = &A[(size_t)j * k];
            for (int t = 0; t < j; t++)
                v -= ri[t] * rj[t];
            A[(size_t)i * k + j] = v / l;
        }
    }
    for (int c = 0; c < nrhs; c++)
    {
        for (int i = 0; i < k; i++)
        {
            S v = b[(size_t)i * nrhs + c];
            for (int t = 0; t < i; t++)
                v -= A[(size_t)i * k + t] * b[(size_t)t * nrhs + c];
            b[(size_t)i * nrhs + c] = v / A[(size_t)i * k + i];
        }
        for (int i = k - 1; i >= 0; i--)
        {
            S v = b[(size_t)i * nrhs + c];
            for (int t = i + 1; t < k; t++)
                v -= A[(size_t)t * k + i] * b[(size_t)t * nrhs + c];
            b[(size_t)i * nrhs + c] = v / A[(size_t)i * k + i];
        }
    }
    return true;
}

template <typename S>
int relaxp_eval(const ochip_relaxp_desc *d, int structure_only, int raw, int mutate, int mutate_arg, const double *delta,
                int *n_out, int *N_out, int *rows_out, int32_t *order, double *cost, double *JtJ, double *Jtr, double *J, double *r,
                int32_t *row_blk, uint8_t *touch)
{
    PEval<S> e(*d, structure_only != 0);
    e.raw = raw, e.mutate = mutate, e.mutate_arg = mutate_arg;
    if (n_out)
        *n_out = e.n;
    if (N_out)
        *N_out = e.N;
    if (rows_out)
        *rows_out = 4 * (int)d->n_points + (e.mono ? 10 : 0);
    if (order)
    {
        int at = 0;
        for (int t : e.cam_t)
            order[at++] = t;
        for (int k = 0; k < 8; k++)
            order[at++] = e.lens_t[k];
    }
    if (!cost && !JtJ && !Jtr && !J && !r && !row_blk && !touch)
        return 0;
    if (delta)
    {
        std::vector<S> dl(delta, delta + e.N);
        e.plus(dl.data());
    }
    e.run();
    if (cost)
        *cost = (double)e.cost;
    to_double(e.JtJ, JtJ);
    to_double(e.Jtr, Jtr);
    to_double(e.J, J);
    to_double(e.r, r);
    if (row_blk)
        std::copy(e.row_blk.begin(), e.row_blk.end(), row_blk);
    if (touch)
        std::copy(e.touch.begin(), e.touch.end(), touch);
    return e.failed ? 1 : 0;
}

// One LM step from the full normal equations (the head of this file): every column scaled and damped as
// LevenbergMarquardtStrategy does, one dense Cholesky solve of all N unknowns, nothing eliminated.
template <typename S>
int relaxp_step(const ochip_relaxp_desc *d, int structure_only, int mutate, int mutate_arg, double radius, const double *scale_c,
                const double *y_test, double *scale_out, double *D2_out, double *y_out, double *delta_out, double *Sc_out,
                double *rhs_c_out, double *Mpp_out, double *cam_q2, double *model2, double *X2, double *scal)
{
    using std::sqrt;
    PEval<S> e(*d, structure_only != 0);
    e.mutate = mutate == PMUT_PARTIAL || mutate == PMUT_NO_CORR_J ? mutate : PMUT_NONE;
    e.mutate_arg = mutate_arg;
    e.run();
    if (e.failed)
        return 1;
    const int n = e.n, N = e.N, P = (int)d->n_points;
    // 1. Jacobi scaling over every column (the reduced unknowns' may be given), 2. the damping
    std::vector<S> s(N), D2(N), M((size_t)N * N), b(N);
    for (int i = 0; i < N; i++)
    {
        const S dg = e.JtJ[(size_t)i * N + i];
        s[i] = i < n && scale_c ? S(scale_c[i]) : S(1) / (S(1) + sqrt(dg));
        const S v = dg * s[i] * s[i];
        D2[i] = std::min(std::max(v, S(1e-6)), S(1e32)) / S(radius);
        if (mutate == PMUT_NO_POINT_DAMPING && i >= n)
            D2[i] = 0;
    }
    // 3. M = S J'J S + D^2, b = S J'r
    for (int i = 0; i < N; i++)
    {
        for (int j = 0; j < N; j++)
            M[(size_t)i * N + j] = e.JtJ[(size_t)i * N + j] * s[i] * s[j];
        M[(size_t)i * N + i] += D2[i];
        b[i] = e.Jtr[i] * s[i];
    }
    // 4. the dense solve of all unknowns, 5. delta = -S y
    std::vector<S> L = M, y = b;
    if (!chol_solve<S>(L, N, y.data(), 1))
        return 1;
    L.clear();
    L.shrink_to_fit();
    std::vector<S> delta(N);
    for (int i = 0; i < N; i++)
        delta[i] = -s[i] * y[i];
    // 6. model cost change = -(step' S g + step' S J'J S step / 2) with step = -y, 7. g . delta
    S sg = 0, quad = 0, gd = 0, gd_p = 0;
    for (int i = 0; i < N; i++)
    {
        sg += -y[i] * b[i];
        S row = 0;
        for (int j = 0; j < N; j++)
            row += (M[(size_t)i * N + j] - (i == j ? D2[i] : S(0))) * -y[j];
        quad += -y[i] * row;
        gd += e.Jtr[i] * delta[i];
        if (i >= n)
            gd_p += e.Jtr[i] * delta[i];
    }
    const S model_cost_change = -(sg + quad / S(2));
    // 8. the candidate: quaternion plus, the focal bounds, the points; |x - candidate|^2 and |candidate|^2 over the
    // variable parameter blocks in ambient coordinates
    PEval<S> cand(*d, structure_only != 0);
    cand.plus(delta.data());
    if (e.lens_t[0] >= 0 && d->opt_focal)
        cand.m[0] = std::min(std::max(cand.m[0], S(d->focal_lo)), S(d->focal_hi));
    S step_sq = 0, cand_sq = 0;
    for (uint32_t c = 0; c < d->n_cams; c++)
        if (e.cam_t[c] >= 0)
            for (int k = 0; k < 4; k++)
            {
                const S a = e.q[4 * c + k], v = cand.q[4 * c + k];
                step_sq += (a - v) * (a - v), cand_sq += v * v;
            }
    for (int blk = 0; blk < 4; blk++)
        if (e.lens_block_variable(blk))
            for (int k = 0; k < PEval<S>::blk_size[blk]; k++)
            {
                const S a = e.m[PEval<S>::blk_first[blk] + k], v = cand.m[PEval<S>::blk_first[blk] + k];
                step_sq += (a - v) * (a - v), cand_sq += v * v;
            }
    for (size_t i = 0; i < e.X.size(); i++)
    {
        const S a = e.X[i], v = cand.X[i];
        step_sq += (a - v) * (a - v), cand_sq += v * v;
    }
    // the Schur complement M_cc - M_cp M_pp^-1 M_pc and the reduced right-hand side b_c - M_cp M_pp^-1 b_p, by dense
    // operations on the full M: M_pp is block diagonal (a point shares no residual with another) - checked
    std::vector<S> Sc((size_t)n * n), rhs(n);
    for (int i = 0; i < n; i++)
    {
        for (int j = 0; j < n; j++)
            Sc[(size_t)i * n + j] = M[(size_t)i * N + j];
        rhs[i] = b[i];
    }
    bool ok = true;
    for (int p = 0; p < P; p++)
    {
        const int t = n + 3 * p;
        for (int a = 0; a < 3; a++)
            for (int j = n; j < N; j++)
                if ((j < t || j >= t + 3) && M[(size_t)(t + a) * N + j] != S(0))
                    ok = false;
        if (Mpp_out)
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++)
                    Mpp_out[9 * (size_t)p + 3 * a + c] = (double)M[(size_t)(t + a) * N + t + c];
        if (mutate == PMUT_DROP_SCHUR && p == mutate_arg)
            continue;
        // Z = M_pp^-1 [M_pc | b_p] (3 x (n + 1))
        std::vector<S> B(9), Z((size_t)3 * (n + 1));
        for (int a = 0; a < 3; a++)
        {
            for (int c = 0; c < 3; c++)
                B[3 * a + c] = M[(size_t)(t + a) * N + t + c];
            for (int j = 0; j < n; j++)
                Z[(size_t)a * (n + 1) + j] = M[(size_t)(t + a) * N + j];
            Z[(size_t)a * (n + 1) + n] = b[t + a];
        }
        if (!chol_solve<S>(B, 3, Z.data(), n + 1))
            return 1;
        for (int i = 0; i < n; i++)
        {
            S w[3];
            bool any = false;
            for (int a = 0; a < 3; a++)
                w[a] = M[(size_t)i * N + t + a], any |= w[a] != S(0);
            if (!any)
                continue;
            for (int j = 0; j <= n; j++)
            {
                const S v = w[0] * Z[j] + w[1] * Z[(size_t)(n + 1) + j] + w[2] * Z[(size_t)2 * (n + 1) + j];
                if (j < n)
                    Sc[(size_t)i * n + j] -= v;
                else
                    rhs[i] -= v;
            }
        }
    }
    if (!ok)
        return 1;
    // the normwise backward error of a given full step y_test (scaled unknowns) on this system
    S berr = 0, Minf = 0, binf = 0, yinf = 0;
    if (y_test)
    {
        S rinf = 0;
        for (int i = 0; i < N; i++)
        {
            S row = 0, res = b[i];
            for (int j = 0; j < N; j++)
            {
                row += std::abs(M[(size_t)i * N + j]);
                res -= M[(size_t)i * N + j] * S(y_test[j]);
            }
            Minf = std::max(Minf, row);
            rinf = std::max(rinf, std::abs(res));
            binf = std::max(binf, std::abs(b[i]));
            yinf = std::max(yinf, std::abs(S(y_test[i])));
        }
        berr = rinf / (Minf * yinf + binf);
    }
    to_double(s, scale_out);
    to_double(D2, D2_out);
    to_double(y, y_out);
    to_double(delta, delta_out);
    to_double(Sc, Sc_out);
    to_double(rhs, rhs_c_out);
    to_double(cand.q, cam_q2);
    to_double(cand.m, model2);
    to_double(cand.X, X2);
    if (scal)
    {
        scal[0] = (double)model_cost_change, scal[1] = (double)step_sq, scal[2] = (double)cand_sq, scal[3] = (double)gd;
        scal[4] = (double)gd_p, scal[5] = (double)berr, scal[6] = 0, scal[7] = 0;
    }
    return 0;
}

} // namespace
} // namespace oracle

extern "C"
{

// One evaluation (see the head of this file).  precision: 0 = double, 1 = long double.  raw: no loss, no corrector (the
// plain residuals and their Jacobian, for the difference quotients).  mutate / mutate_arg: PMUT_* above.  delta (N or
// NULL): the state moved by x [+] delta first.  n_out: the reduced unknowns, N_out = n + 3 n_points, rows_out the rows of
// J; order (n_cams + 8): the first canonical column of every camera, then of f ppx ppy k1 k2 k3 p1 p2, or -1.  Outputs
// may be NULL (all of cost .. touch NULL: the sizes and the order only).  Returns 1 when a block did not evaluate to
// finite values, else 0.
int oc_relaxp_eval(const ochip_relaxp_desc *d, int structure_only, int precision, int raw, int mutate, int mutate_arg,
                   const double *delta, int *n_out, int *N_out, int *rows_out, int32_t *order, double *cost, double *JtJ, double *Jtr,
                   double *J, double *r, int32_t *row_blk, uint8_t *touch)
{
    if (precision)
        return oracle::relaxp_eval<long double>(d, structure_only, raw, mutate, mutate_arg, delta, n_out, N_out, rows_out, order, cost,
                                                JtJ, Jtr, J, r, row_blk, touch);
    return oracle::relaxp_eval<double>(d, structure_only, raw, mutate, mutate_arg, delta, n_out, N_out, rows_out, order, cost, JtJ, Jtr,
                                       J, r, row_blk, touch);
}

// One LM step at trust-region radius `radius` from the full system.  scale_c (n or NULL): the Jacobi scaling of the
// reduced unknowns (NULL: 1 / (1 + sqrt(diag)) like every other column).  y_test (N or NULL): a full step in scaled
// unknowns whose backward error |b - M y| / (|M| |y| + |b|) (infinity norms) goes to scal[5].  Outputs (any may be
// NULL): scale, D2, y, delta (N each; delta = -scale y), Sc (n x n) the Schur complement of the point blocks in M and
// rhs_c (n) the reduced right-hand side, Mpp (n_points x 9) the damped point blocks, the candidate state cam_q2
// (n_cams x 4), model2 (8), X2 (n_points x 3); scal[8]: [0] model cost change, [1] |x - candidate|^2, [2] |candidate|^2,
// [3] g . delta, [4] the points' share of it, [5] the backward error.  Returns 1 when the evaluation or a factorisation
// failed.
int oc_relaxp_step(const ochip_relaxp_desc *d, int structure_only, int precision, int mutate, int mutate_arg, double radius,
                   const double *scale_c, const double *y_test, double *scale, double *D2, double *y, double *delta, double *Sc,
                   double *rhs_c, double *Mpp, double *cam_q2, double *model2, double *X2, double *scal)
{
    if (precision)
        return oracle::relaxp_step<long double>(d, structure_only, mutate, mutate_arg, radius, scale_c, y_test, scale, D2, y, delta, Sc,
                                                rhs_c, Mpp, cam_q2, model2, X2, scal);
    return oracle::relaxp_step<double>(d, structure_only, mutate, mutate_arg, radius, scale_c, y_test, scale, D2, y, delta, Sc, rhs_c,
                                       Mpp, cam_q2, model2, X2, scal);
}

// Richardson-extrapolated central differences in long double of the raw residuals over the canonical columns:
// D(h) = (r(x [+] h e_j) - r(x [+] -h e_j)) / 2h, Jfd = (4 D(h/2) - D(h)) / 3, with h = step * max(1, |x_j|) for the
// Euclidean unknowns and h = step for the quaternion tangents.  Jfd: rows x N.
int oc_relaxp_fd(const ochip_relaxp_desc *d, int structure_only, double step, double *Jfd)
{
    using S = long double;
    oracle::PEval<S> base(*d, structure_only != 0);
    const int N = base.N;
    std::vector<S> scale(N, S(1));
    for (int k = 0; k < 8; k++)
        if (base.lens_t[k] >= 0)
            scale[base.lens_t[k]] = std::max<S>(1, std::abs(base.m[k]));
    for (size_t i = 0; i < base.X.size(); i++)
        scale[base.n + i] = std::max<S>(1, std::abs(base.X[i]));
    auto residuals = [&](int j, S h) {
        oracle::PEval<S> e(*d, structure_only != 0);
        e.raw = 1;
        std::vector<S> dl(N, S(0));
        dl[j] = h;
        e.plus(dl.data());
        e.run();
        return e.r;
    };
    int failed = 0;
    for (int j = 0; j < N; j++)
    {
        const S h = S(step) * scale[j];
        const std::vector<S> a = residuals(j, h), b = residuals(j, -h), c = residuals(j, h / 2), e = residuals(j, -h / 2);
        const size_t rows = a.size();
        for (size_t i = 0; i < rows; i++)
        {
            const S d1 = (a[i] - b[i]) / (2 * h), d2 = (c[i] - e[i]) / h;
            const S v = (4 * d2 - d1) / 3;
            failed |= !std::isfinite(v);
            Jfd[i * N + j] = (double)v;
        }
    }
    return failed;
}

} // extern "C"
