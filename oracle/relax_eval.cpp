// ORACLE — test infrastructure only (see oracle.hpp).
//
// One evaluation of the general engine's problem (the flat ochip_relaxg_desc the device takes) the way the reference's
// Problem evaluates it: every residual block through the restated functors on Jets of a selectable scalar (double, or
// long double for a reference with 11 more bits), the EigenQuaternionManifold / SubsetManifold plus-Jacobians, HuberLoss
// and the Triggs corrector, then J'J, J'r and the cost summed in that scalar.  tests/test_relax_eval_oracle.py checks it
// against its own central differences; tests/test_gpu_relax_eval.py compares the device's evaluation with it.
//
// Residual blocks, in this order (the row order of J):
//   ray blocks in the caller's order: 2 rays PlaneIntersectionAngleCost / TwoRayFocalRadial with HuberLoss(huber_a),
//   3..5 rays NRay / NRayFocalRadial without a loss; PointsDownwardsPrior per down_cam; DifferenceCost per diff_v pair;
//   DifferenceCost of every vertex against its initial height when anchor_weight != 0; AdjacentTriangleNormalCost per
//   smooth_v quadruple; DistortionMonotonicityCost when mono_observations > 0; MultiDecomposedRotationCost with
//   HuberLoss(rel_huber_a) per relation.
// Canonical unknown order (the column order): 3 per variable camera in index order, 1 per variable vertex in index order,
// then f, (ppx, ppy), k1 .. k_n_radial_free.  A group is variable when it is optimised (cameras and intrinsics: and not
// structure_only) and some block reads it - the reference's reduced program.
#include "../include/ochip.h"
#include "mini_ceres.hpp"
#include "relax_functors.hpp"

#include <cstring>
#include <vector>

namespace oracle
{
namespace
{

enum
{
    K_EUCL = 0,
    K_QUAT = 1,
    K_RADIAL = 2 // SubsetManifold: the leading n_radial_free coefficients variable
};

template <typename S> struct Slot
{
    const S *val;
    int size, kind, t; // t: first canonical column, -1 = constant
};

// perturbations of the evaluation, for the tests that show the bounds bite
enum
{
    MUT_NONE = 0,
    MUT_PARTIAL = 1,   // block `arg`: its largest corrected partial times (1 + 1e-9)
    MUT_NO_CORR_J = 2, // the corrector applied to the residuals of a loss block but not to its Jacobian
    MUT_DROP = 3       // block `arg` left out of J'J and J'r (its cost kept)
};

template <typename S> struct GEval
{
    const ochip_relaxg_desc &d;
    bool structure_only;
    int raw = 0, mutate = MUT_NONE, mutate_arg = -1;
    std::vector<S> q, z, z0, m;
    std::vector<int> cam_t, vert_t;
    int f_t = -1, pp_t = -1, k_t = -1, nk = 0, n = 0, rows = 0;
    // outputs (rows x n, row-major)
    std::vector<S> J, r, JtJ, Jtr;
    std::vector<int32_t> row_blk;
    std::vector<uint8_t> touch;
    S cost = 0, cost_reduced = 0; // every block / the blocks that read at least one unknown (Ceres' reduced program)
    bool failed = false;

    GEval(const ochip_relaxg_desc &d_, bool so) : d(d_), structure_only(so)
    {
        q.assign(d.cam_q, d.cam_q + 4 * (size_t)d.n_cams);
        z.assign(d.vert_z, d.vert_z + d.n_verts);
        z0 = z;
        m.assign(d.model, d.model + 8);
        nk = std::min<int>(d.n_radial_free, 3);
        layout();
    }
    uint32_t n_anchor() const
    {
        return d.anchor_weight != 0.0 ? d.n_verts : 0;
    }
    bool intr(uint32_t b) const
    {
        return d.blk_intr && d.blk_intr[b];
    }
    void layout()
    {
        const uint32_t nc = d.n_cams, nv = d.n_verts;
        std::vector<char> cam_used(nc, 0), vert_used(nv, 0);
        bool f_used = false, k_used = false;
        for (uint32_t b = 0; b < d.n_blocks; b++)
        {
            for (uint32_t i = d.blk_ray_off[b]; i < d.blk_ray_off[b + 1]; i++)
                cam_used[d.ray_cam[i]] = 1;
            for (int j = 0; j < 3; j++)
                vert_used[d.blk_tri[3 * (size_t)b + j]] = 1;
            f_used |= intr(b);
            rows += 3 * d.blk_n[b];
        }
        k_used = f_used || d.mono_observations > 0;
        for (uint32_t i = 0; i < d.n_down; i++)
            cam_used[d.down_cam[i]] = 1;
        for (uint32_t i = 0; i < 2 * d.n_diff; i++)
            vert_used[d.diff_v[i]] = 1;
        for (uint32_t i = 0; i < n_anchor(); i++)
            vert_used[i] = 1;
        for (uint32_t i = 0; i < 4 * d.n_smooth; i++)
            vert_used[d.smooth_v[i]] = 1;
        for (uint32_t i = 0; i < 2 * d.n_rel; i++)
            cam_used[d.rel_cam[i]] = 1;
        rows += d.n_down + d.n_diff + n_anchor() + d.n_smooth + (d.mono_observations > 0 ? 10 : 0) + 3 * d.n_rel;
        cam_t.assign(nc, -1);
        vert_t.assign(nv, -1);
        for (uint32_t c = 0; c < nc; c++)
            if (d.cam_optimize[c] && !structure_only && cam_used[c])
                cam_t[c] = n, n += 3;
        for (uint32_t v = 0; v < nv; v++)
            if (d.vert_optimize[v] && vert_used[v])
                vert_t[v] = n++;
        if (d.opt_focal && !structure_only && f_used)
            f_t = n++;
        if (d.opt_principal && !structure_only && f_used)
            pp_t = n, n += 2;
        if (nk > 0 && !structure_only && k_used)
            k_t = n, n += nk;
    }
    // x <- x [+] delta over the canonical unknowns
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
        for (uint32_t v = 0; v < d.n_verts; v++)
            if (vert_t[v] >= 0)
                z[v] += delta[vert_t[v]];
        if (f_t >= 0)
            m[0] += delta[f_t];
        if (pp_t >= 0)
            m[1] += delta[pp_t], m[2] += delta[pp_t + 1];
        for (int k = 0; k < nk && k_t >= 0; k++)
            m[3 + k] += delta[k_t + k];
    }

    // one block: residuals and ambient Jacobian on Jet<K, S>, then the tangent rows, the loss and the assembly
    template <int K, typename F> void block(int b, int nr, const std::vector<Slot<S>> &slots, const mc::HuberLoss *loss, F &&call)
    {
        using J_t = Jet<K, S>;
        std::vector<J_t> x(K);
        std::vector<const J_t *> ptr(slots.size());
        int off = 0;
        for (size_t s = 0; s < slots.size(); s++)
        {
            ptr[s] = x.data() + off;
            for (int k = 0; k < slots[s].size; k++)
                x[off + k] = J_t(slots[s].val[k], off + k);
            off += slots[s].size;
        }
        J_t out[15];
        bool ok = call(ptr.data(), out);
        const int row0 = (int)r.size();
        std::vector<S> Jb((size_t)nr * n, S(0));
        std::vector<uint8_t> tb((size_t)nr * n, 0);
        S sq = 0;
        for (int i = 0; i < nr; i++)
        {
            r.push_back(out[i].a);
            row_blk.push_back(b);
            sq += out[i].a * out[i].a;
            ok &= std::isfinite(out[i].a);
            off = 0;
            for (const Slot<S> &sl : slots)
            {
                if (sl.t >= 0)
                {
                    if (sl.kind == K_QUAT)
                    {
                        if constexpr (K >= 4) // (the blocks with fewer ambient parameters have no quaternion)
                        {
                            S PJ[12];
                            mc::quat_plus_jacobian_t<S>(sl.val, PJ);
                            for (int c = 0; c < 3; c++)
                            {
                                S v = 0;
                                for (int k = 0; k < 4; k++)
                                    v += out[i].v[off + k] * PJ[k * 3 + c];
                                Jb[(size_t)i * n + sl.t + c] += v;
                                tb[(size_t)i * n + sl.t + c] = 1;
                            }
                        }
                    }
                    else
                    {
                        const int cols = sl.kind == K_RADIAL ? nk : sl.size;
                        for (int c = 0; c < cols; c++)
                        {
                            Jb[(size_t)i * n + sl.t + c] += out[i].v[off + c];
                            tb[(size_t)i * n + sl.t + c] = 1;
                        }
                    }
                }
                off += sl.size;
            }
        }
        for (S v : Jb)
            ok &= std::isfinite(v);
        failed |= !ok;
        S rho[3] = {sq, S(1), S(0)};
        if (loss && !raw)
            mc::huber_rho<S>(S(loss->a), S(loss->b), sq, rho);
        cost += S(0.5) * rho[0];
        bool reads_unknown = false;
        for (const Slot<S> &sl : slots)
            reads_unknown |= sl.t >= 0;
        if (reads_unknown)
            cost_reduced += S(0.5) * rho[0];
        if (loss && !raw)
        {
            S sqrt_rho1, scaling, alpha_sq_norm;
            mc::corrector_terms<S>(sq, rho, &sqrt_rho1, &scaling, &alpha_sq_norm);
            if (mutate != MUT_NO_CORR_J)
                for (int c = 0; c < n; c++)
                {
                    S rtj = 0;
                    for (int i = 0; i < nr; i++)
                        rtj += Jb[(size_t)i * n + c] * r[row0 + i];
                    for (int i = 0; i < nr; i++)
                        Jb[(size_t)i * n + c] = sqrt_rho1 * (Jb[(size_t)i * n + c] - alpha_sq_norm * r[row0 + i] * rtj);
                }
            for (int i = 0; i < nr; i++)
                r[row0 + i] *= scaling;
        }
        if (mutate == MUT_PARTIAL && b == mutate_arg)
        {
            size_t at = 0;
            for (size_t e = 0; e < Jb.size(); e++)
                if (std::abs(Jb[e]) > std::abs(Jb[at]))
                    at = e;
            Jb[at] *= S(1) + S(1e-9);
        }
        J.insert(J.end(), Jb.begin(), Jb.end());
        touch.insert(touch.end(), tb.begin(), tb.end());
        if (mutate == MUT_DROP && b == mutate_arg)
            return;
        for (int i = 0; i < nr; i++)
        {
            const S *row = &Jb[(size_t)i * n];
            for (int a = 0; a < n; a++)
            {
                if (row[a] == S(0))
                    continue;
                Jtr[a] += row[a] * r[row0 + i];
                for (int c = 0; c < n; c++)
                    JtJ[(size_t)a * n + c] += row[a] * row[c];
            }
        }
    }

    Slot<S> cam(uint32_t c)
    {
        return {&q[4 * (size_t)c], 4, K_QUAT, cam_t[c]};
    }
    Slot<S> vert(uint32_t v)
    {
        return {&z[v], 1, K_EUCL, vert_t[v]};
    }

    template <int N> void ray_block(uint32_t b, const mc::HuberLoss *loss)
    {
        MultiRayCost<N> c;
        const uint32_t r0 = d.blk_ray_off[b];
        std::vector<Slot<S>> slots;
        for (int i = 0; i < N; i++)
        {
            const uint32_t cm = d.ray_cam[r0 + i];
            for (int k = 0; k < 3; k++)
            {
                c.camera_loc[i][k] = d.cam_pos[3 * (size_t)cm + k];
                c.camera_ray[i][k] = d.ray_dir ? d.ray_dir[3 * (size_t)(r0 + i) + k] : NAN;
            }
            for (int k = 0; k < 2; k++)
                c.camera_pixel[i][k] = d.ray_px ? d.ray_px[2 * (size_t)(r0 + i) + k] : NAN;
            slots.push_back(cam(cm));
        }
        for (int j = 0; j < 3; j++)
        {
            const uint32_t v = d.blk_tri[3 * (size_t)b + j];
            c.plane_point[j][0] = d.vert_xy[2 * (size_t)v];
            c.plane_point[j][1] = d.vert_xy[2 * (size_t)v + 1];
            slots.push_back(vert(v));
        }
        c.shared_tangential[0] = d.model[6];
        c.shared_tangential[1] = d.model[7];
        const int R = 3 * N;
        if (!intr(b))
        {
            if constexpr (N == 2)
            {
                PlaneIntersectionAngleCost p;
                std::memcpy(p.camera_loc, c.camera_loc, sizeof p.camera_loc);
                std::memcpy(p.camera_ray, c.camera_ray, sizeof p.camera_ray);
                std::memcpy(p.plane_point, c.plane_point, sizeof p.plane_point);
                block<4 * N + 3>(b, R, slots, loss, [&](auto p_, auto o) { return p(p_[0], p_[1], p_[2], p_[3], p_[4], o); });
            }
            else
                block<4 * N + 3>(b, R, slots, loss, [&](auto p_, auto o) {
                    using T = std::remove_const_t<std::remove_pointer_t<std::remove_pointer_t<decltype(p_)>>>;
                    const T *rot[N];
                    for (int i = 0; i < N; i++)
                        rot[i] = p_[i];
                    return c.template computeResiduals<T>(rot, p_[N], p_[N + 1], p_[N + 2], o);
                });
            return;
        }
        slots.push_back({&m[0], 1, K_EUCL, f_t});
        slots.push_back({&m[1], 2, K_EUCL, pp_t});
        slots.push_back({&m[3], 3, K_RADIAL, k_t});
        block<4 * N + 9>(b, R, slots, loss, [&](auto p_, auto o) {
            using T = std::remove_const_t<std::remove_pointer_t<std::remove_pointer_t<decltype(p_)>>>;
            const T *rot[N];
            for (int i = 0; i < N; i++)
                rot[i] = p_[i];
            return c.template computeResidualsFocalRadial<T>(rot, p_[N], p_[N + 1], p_[N + 2], p_[N + 3], p_[N + 4], p_[N + 5], o);
        });
    }

    void run()
    {
        J.clear(), r.clear(), row_blk.clear(), touch.clear();
        JtJ.assign((size_t)n * n, S(0));
        Jtr.assign(n, S(0));
        cost = cost_reduced = 0;
        failed = false;
        const mc::HuberLoss huber(d.huber_a), rel_huber(d.rel_huber_a);
        int b = 0;
        for (uint32_t i = 0; i < d.n_blocks; i++, b++)
            switch (d.blk_n[i])
            {
            case 2:
                ray_block<2>(i, &huber);
                break;
            case 3:
                ray_block<3>(i, nullptr);
                break;
            case 4:
                ray_block<4>(i, nullptr);
                break;
            default:
                ray_block<5>(i, nullptr);
                break;
            }
        for (uint32_t i = 0; i < d.n_down; i++, b++)
        {
            PointsDownwardsPrior f(d.down_weight);
            block<4>(b, 1, {cam(d.down_cam[i])}, nullptr, [&](auto p, auto o) { return f(p[0], o); });
        }
        for (uint32_t i = 0; i < d.n_diff; i++, b++)
        {
            DifferenceCost f(d.diff_weight);
            block<2>(b, 1, {vert(d.diff_v[2 * i]), vert(d.diff_v[2 * i + 1])}, nullptr, [&](auto p, auto o) { return f(p[0], p[1], o); });
        }
        for (uint32_t i = 0; i < n_anchor(); i++, b++)
        {
            DifferenceCost f(d.anchor_weight);
            block<2>(b, 1, {vert(i), {&z0[i], 1, K_EUCL, -1}}, nullptr, [&](auto p, auto o) { return f(p[0], p[1], o); });
        }
        for (uint32_t i = 0; i < d.n_smooth; i++, b++)
        {
            AdjacentTriangleNormalCost f;
            double *xy[4] = {f.xyA, f.xyB, f.xyC, f.xyD};
            std::vector<Slot<S>> slots;
            for (int a = 0; a < 4; a++)
            {
                const uint32_t v = d.smooth_v[4 * i + a];
                xy[a][0] = d.vert_xy[2 * (size_t)v], xy[a][1] = d.vert_xy[2 * (size_t)v + 1];
                slots.push_back(vert(v));
            }
            f.weight = d.smooth_weight;
            block<4>(b, 1, slots, nullptr, [&](auto p, auto o) { return f(p[0], p[1], p[2], p[3], o); });
        }
        if (d.mono_observations > 0)
        {
            DistortionMonotonicityCost f;
            f.r_max = d.mono_r_max;
            f.weight = std::sqrt(d.mono_observations / 10.0);
            block<3>(b, 10, {{&m[3], 3, K_RADIAL, k_t}}, nullptr, [&](auto p, auto o) { return f(p[0], o); });
            b++;
        }
        for (uint32_t i = 0; i < d.n_rel; i++, b++)
        {
            const uint32_t c1 = d.rel_cam[2 * i], c2 = d.rel_cam[2 * i + 1];
            std::array<decomposed_pose, 4> poses;
            for (int k = 0; k < 4; k++)
            {
                const double *e = d.rel_pose + 32 * (size_t)i + 8 * k;
                poses[k].orientation = {e[0], e[1], e[2], e[3]};
                poses[k].position = {e[4], e[5], e[6]};
                poses[k].score = (int)e[7];
            }
            const double *p1 = d.cam_pos + 3 * (size_t)c1, *p2 = d.cam_pos + 3 * (size_t)c2;
            MultiDecomposedRotationCost f(poses, {p1[0], p1[1], p1[2]}, {p2[0], p2[1], p2[2]});
            block<8>(b, 3, {cam(c1), cam(c2)}, &rel_huber, [&](auto p, auto o) { return f(p[0], p[1], o); });
        }
    }
};

template <typename S> void to_double(const std::vector<S> &v, double *out)
{
    if (out)
        for (size_t i = 0; i < v.size(); i++)
            out[i] = (double)v[i];
}

template <typename S>
int relaxg_eval(const ochip_relaxg_desc *d, int structure_only, int raw, int mutate, int mutate_arg, const double *delta,
                int *n_out, int *rows_out, int32_t *order, double *cost, double *JtJ, double *Jtr, double *J, double *r,
                int32_t *row_blk, uint8_t *touch, double *cost_reduced)
{
    GEval<S> e(*d, structure_only != 0);
    e.raw = raw, e.mutate = mutate, e.mutate_arg = mutate_arg;
    if (delta)
    {
        std::vector<S> dl(delta, delta + e.n);
        e.plus(dl.data());
    }
    e.run();
    if (n_out)
        *n_out = e.n;
    if (rows_out)
        *rows_out = (int)e.r.size();
    if (order)
    {
        int at = 0;
        for (int t : e.cam_t)
            order[at++] = t;
        for (int t : e.vert_t)
            order[at++] = t;
        order[at++] = e.f_t, order[at++] = e.pp_t, order[at++] = e.k_t;
    }
    if (cost)
        *cost = (double)e.cost;
    if (cost_reduced)
        *cost_reduced = (double)e.cost_reduced;
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

} // namespace
} // namespace oracle

extern "C"
{

// One evaluation (see the head of this file).  precision: 0 = double, 1 = long double.  raw: no loss, no corrector (the
// plain residuals and their Jacobian, for the difference quotients).  mutate / mutate_arg: MUT_* above.  delta (n or NULL):
// the state moved by x [+] delta first.  Outputs may be NULL; n_out / rows_out size them (J and touch: rows x n).
// Returns 1 when a block did not evaluate to finite values (the reference's Problem fails the evaluation), else 0.
int oc_relaxg_eval(const ochip_relaxg_desc *d, int structure_only, int precision, int raw, int mutate, int mutate_arg,
                   const double *delta, int *n_out, int *rows_out, int32_t *order, double *cost, double *JtJ, double *Jtr,
                   double *J, double *r, int32_t *row_blk, uint8_t *touch)
{
    if (precision)
        return oracle::relaxg_eval<long double>(d, structure_only, raw, mutate, mutate_arg, delta, n_out, rows_out, order, cost,
                                                JtJ, Jtr, J, r, row_blk, touch, nullptr);
    return oracle::relaxg_eval<double>(d, structure_only, raw, mutate, mutate_arg, delta, n_out, rows_out, order, cost, JtJ,
                                       Jtr, J, r, row_blk, touch, nullptr);
}

// oc_relaxg_eval, and the cost of the reduced program: the blocks that read at least one unknown (cost_reduced, may be
// NULL).  The plane engine and the chain leave the others out, as Ceres' reduced program does; `cost` counts every block.
int oc_relaxg_eval_reduced(const ochip_relaxg_desc *d, int structure_only, int precision, int raw, int mutate, int mutate_arg,
                           const double *delta, int *n_out, int *rows_out, int32_t *order, double *cost, double *JtJ, double *Jtr,
                           double *J, double *r, int32_t *row_blk, uint8_t *touch, double *cost_reduced)
{
    if (precision)
        return oracle::relaxg_eval<long double>(d, structure_only, raw, mutate, mutate_arg, delta, n_out, rows_out, order, cost,
                                                JtJ, Jtr, J, r, row_blk, touch, cost_reduced);
    return oracle::relaxg_eval<double>(d, structure_only, raw, mutate, mutate_arg, delta, n_out, rows_out, order, cost, JtJ,
                                       Jtr, J, r, row_blk, touch, cost_reduced);
}

// Richardson-extrapolated central differences in long double of the raw residuals over the canonical unknowns:
// D(h) = (r(x [+] h e_j) - r(x [+] -h e_j)) / 2h, Jfd = (4 D(h/2) - D(h)) / 3, with h = step * max(1, |x_j|) for the
// Euclidean unknowns and h = step for the quaternion tangents.  Jfd: rows x n.
int oc_relaxg_fd(const ochip_relaxg_desc *d, int structure_only, double step, double *Jfd)
{
    using S = long double;
    oracle::GEval<S> base(*d, structure_only != 0);
    const int n = base.n;
    std::vector<S> scale(n, S(1));
    for (uint32_t v = 0; v < d->n_verts; v++)
        if (base.vert_t[v] >= 0)
            scale[base.vert_t[v]] = std::max<S>(1, std::abs(base.z[v]));
    if (base.f_t >= 0)
        scale[base.f_t] = std::max<S>(1, std::abs(base.m[0]));
    if (base.pp_t >= 0)
        for (int k = 0; k < 2; k++)
            scale[base.pp_t + k] = std::max<S>(1, std::abs(base.m[1 + k]));
    auto residuals = [&](int j, S h) {
        oracle::GEval<S> e(*d, structure_only != 0);
        e.raw = 1;
        std::vector<S> dl(n, S(0));
        dl[j] = h;
        e.plus(dl.data());
        e.run();
        return e.r;
    };
    int failed = 0;
    for (int j = 0; j < n; j++)
    {
        const S h = S(step) * scale[j];
        const std::vector<S> a = residuals(j, h), b = residuals(j, -h), c = residuals(j, h / 2), e = residuals(j, -h / 2);
        const size_t rows = a.size();
        for (size_t i = 0; i < rows; i++)
        {
            const S d1 = (a[i] - b[i]) / (2 * h), d2 = (c[i] - e[i]) / h;
            const S v = (4 * d2 - d1) / 3;
            failed |= !std::isfinite(v);
            Jfd[i * n + j] = (double)v;
        }
    }
    return failed;
}

} // extern "C"
