// Host checks of the shared Levenberg-Marquardt step rules (opencalibration_amd/csrc/relax_lm_rules.hpp), built and run by
// tests/test_lm_rules_host.py with the system g++ under the address and undefined-behaviour sanitizers.  Usage:
//   lm_rules_driver quat_plus | quat_normalize | diagonal | trust
#include "../opencalibration_amd/csrc/relax_lm_rules.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>

using namespace ochip;

namespace
{
int failures = 0;
#define CHECK(cond, ...)                                                                                                          \
    do                                                                                                                            \
    {                                                                                                                             \
        if (!(cond))                                                                                                              \
        {                                                                                                                         \
            if (failures++ < 20)                                                                                                  \
            {                                                                                                                     \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);                                                             \
                printf(__VA_ARGS__);                                                                                              \
                printf("\n");                                                                                                     \
            }                                                                                                                     \
        }                                                                                                                         \
    } while (0)

bool same_bits(double a, double b)
{
    return std::memcmp(&a, &b, 8) == 0;
}

void random_unit_quat(std::mt19937_64 &rng, double q[4])
{
    std::normal_distribution<double> g(0.0, 1.0);
    double n2 = 0;
    do
    {
        n2 = 0;
        for (int k = 0; k < 4; k++)
        {
            q[k] = g(rng);
            n2 += q[k] * q[k];
        }
    } while (n2 < 1e-6);
    for (int k = 0; k < 4; k++)
        q[k] /= std::sqrt(n2);
}

// o = exp(d) * q in long double
void quat_plus_ld(const double q[4], const double d[3], long double o[4])
{
    const long double d0 = d[0], d1 = d[1], d2 = d[2];
    const long double nrm = sqrtl(d0 * d0 + d1 * d1 + d2 * d2);
    if (nrm == 0.0L)
    {
        for (int k = 0; k < 4; k++)
            o[k] = q[k];
        return;
    }
    const long double s = sinl(nrm) / nrm;
    const long double dx = s * d0, dy = s * d1, dz = s * d2, dw = cosl(nrm);
    const long double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    o[3] = dw * qw - dx * qx - dy * qy - dz * qz;
    o[0] = dw * qx + dx * qw + dy * qz - dz * qy;
    o[1] = dw * qy + dy * qw + dz * qx - dx * qz;
    o[2] = dw * qz + dz * qw + dx * qy - dy * qx;
}

// Each component is four products of factors <= 1, each carrying ~3.5 ulp (sin / cos, the division, the product), plus
// three additions: ~17 ulp of 2^-53; the bound is twice that.
const double QUAT_PLUS_BOUND = 32.0 * std::ldexp(1.0, -53);

double check_quat_plus(const double q[4], const double d[3])
{
    double o[4];
    long double ref[4];
    lm_quat_plus(q, d, o);
    quat_plus_ld(q, d, ref);
    double worst = 0;
    for (int k = 0; k < 4; k++)
    {
        const double err = (double)fabsl((long double)o[k] - ref[k]);
        worst = std::max(worst, err);
        CHECK(err <= QUAT_PLUS_BOUND, "component %d: %.17g vs %.17Lg (d = %g %g %g)", k, o[k], ref[k], d[0], d[1], d[2]);
    }
    return worst;
}

void test_quat_plus()
{
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::normal_distribution<double> g(0.0, 1.0);
    const double lo = std::log(1e-300), hi = std::log(3.0);
    double worst = 0;
    for (int i = 0; i < 10000; i++)
    {
        double q[4], dir[3], d[3], n2 = 0;
        random_unit_quat(rng, q);
        do
        {
            n2 = 0;
            for (int k = 0; k < 3; k++)
            {
                dir[k] = g(rng);
                n2 += dir[k] * dir[k];
            }
        } while (n2 < 1e-6);
        const double len = std::exp(lo + (hi - lo) * u(rng));
        for (int k = 0; k < 3; k++)
            d[k] = dir[k] / std::sqrt(n2) * len;
        worst = std::max(worst, check_quat_plus(q, d));
    }
    double q[4], o[4];
    random_unit_quat(rng, q);
    const double zero[3] = {0, 0, 0};
    lm_quat_plus(q, zero, o);
    for (int k = 0; k < 4; k++)
        CHECK(same_bits(o[k], q[k]), "d = 0 must return q: component %d", k);
    const double sub[3] = {std::numeric_limits<double>::denorm_min() * 3, 0.0, -std::numeric_limits<double>::denorm_min() * 7};
    worst = std::max(worst, check_quat_plus(q, sub));
    printf("quat_plus: worst error %.3g (bound %.3g)\n", worst, QUAT_PLUS_BOUND);
}

void test_quat_normalize()
{
    double z[4] = {0, 0, 0, 0};
    lm_quat_normalize(z);
    for (int k = 0; k < 4; k++)
        CHECK(same_bits(z[k], 0.0), "a zero quaternion must stay: component %d = %g", k, z[k]);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double qn[4] = {nan, nan, nan, nan};
    lm_quat_normalize(qn);
    for (int k = 0; k < 4; k++)
        CHECK(std::isnan(qn[k]), "NaN must stay NaN: component %d = %g", k, qn[k]);
    double q1[4] = {0.5, nan, 0.5, 0.5};
    lm_quat_normalize(q1);
    CHECK(std::isnan(q1[1]), "a NaN component must stay NaN: %g", q1[1]);

    std::mt19937_64 rng(77);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int i = 0; i < 10000; i++)
    {
        double q[4], e[4];
        random_unit_quat(rng, q);
        const double norm = std::pow(10.0, -150.0 + 300.0 * u(rng));
        for (int k = 0; k < 4; k++)
            q[k] *= norm;
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        for (int k = 0; k < 4; k++)
            e[k] = q[k] / std::sqrt(n2);
        lm_quat_normalize(q);
        for (int k = 0; k < 4; k++)
            CHECK(same_bits(q[k], e[k]), "norm %g component %d: %.17g vs %.17g", norm, k, q[k], e[k]);
    }
    printf("quat_normalize: done\n");
}

void test_diagonal()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(same_bits(lm_clamp_diagonal(0.0), 1e-6), "below");
    CHECK(same_bits(lm_clamp_diagonal(-5.0), 1e-6), "negative");
    CHECK(same_bits(lm_clamp_diagonal(9.9e-7), 1e-6), "just below");
    CHECK(same_bits(lm_clamp_diagonal(1e-6), 1e-6), "lower edge");
    CHECK(same_bits(lm_clamp_diagonal(3.25), 3.25), "inside");
    CHECK(same_bits(lm_clamp_diagonal(1e32), 1e32), "upper edge");
    CHECK(same_bits(lm_clamp_diagonal(1.1e32), 1e32), "above");
    CHECK(same_bits(lm_clamp_diagonal(inf), 1e32), "infinity");
    CHECK(same_bits(lm_clamp_diagonal(-inf), 1e-6), "minus infinity");
    CHECK(std::isnan(lm_clamp_diagonal(nan)), "NaN passes through");
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> u(-40.0, 40.0);
    for (int i = 0; i < 10000; i++)
    {
        const double v = std::pow(10.0, u(rng));
        CHECK(same_bits(lm_clamp_diagonal(v), std::min(std::max(v, 1e-6), 1e32)), "clamp of %g", v);
        CHECK(same_bits(lm_jacobi_scale(v), 1.0 / (1.0 + std::sqrt(v))), "jacobi scale of %g", v);
        const double radius = std::pow(10.0, u(rng) * 0.4);
        const double dd = std::sqrt(v / radius);
        CHECK(same_bits(lm_damping(v, radius), dd * dd), "damping of %g / %g", v, radius);
    }
    CHECK(same_bits(lm_jacobi_scale(0.0), 1.0), "jacobi scale of 0");
    CHECK(same_bits(lm_jacobi_scale(inf), 0.0), "jacobi scale of infinity");
    CHECK(std::isnan(lm_jacobi_scale(nan)) && std::isnan(lm_jacobi_scale(-1.0)), "jacobi scale of NaN / a negative diagonal");
    const ochip_relax_options o = lm_reference_options();
    CHECK(o.max_num_iterations == 100 && o.initial_trust_region_radius == 1.0 && o.function_tolerance == 1e-6 &&
              o.gradient_tolerance == 1e-10 && o.parameter_tolerance == 1e-8,
          "reference options");
    printf("diagonal: done\n");
}

// ---- the trust-region bookkeeping of lm_solve as it stood before the rules were shared, transcribed: the only place
//      where the test restates the rule -------------------------------------------------------------------------------------
enum
{
    EV_ACCEPT,
    EV_REJECT,
    EV_INVALID
};
// returns true when the solve must fail (the fifth invalid step in a row)
bool parent_event(double &radius, double &decrease_factor, int &invalid, int event, double rho)
{
    if (event == EV_INVALID)
    {
        if (++invalid >= 5)
            return true;
        radius *= 0.5;
        return false;
    }
    invalid = 0;
    if (rho > 1e-3)
    {
        const double t = 2.0 * rho - 1.0;
        radius = radius / std::max(1.0 / 3.0, 1.0 - t * t * t);
        radius = std::min(1e16, radius);
        decrease_factor = 2.0;
    }
    else
    {
        radius = radius / decrease_factor;
        decrease_factor *= 2.0;
    }
    return false;
}

void test_trust()
{
    std::mt19937_64 rng(99);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    long events = 0;
    for (int seq = 0; seq < 10000; seq++)
    {
        const double r0 = std::pow(10.0, -4.0 + 8.0 * u(rng));
        lm_trust tr;
        tr.start(r0);
        double radius = r0, decrease = 2.0;
        int invalid = 0;
        CHECK(same_bits(tr.radius, radius) && same_bits(tr.decrease, decrease) && tr.invalid == 0, "start");
        const int len = 1 + (int)(u(rng) * 60);
        // (sequences lean to one kind of event so that runs of rejections reach the radius floor and runs of invalid steps
        // reach the fifth)
        const double p_invalid = u(rng) * u(rng), p_reject = u(rng);
        for (int e = 0; e < len; e++)
        {
            const double x = u(rng);
            const int ev = x < p_invalid ? EV_INVALID : (u(rng) < p_reject ? EV_REJECT : EV_ACCEPT);
            // accepted: rho in (1e-3, 2]; rejected: rho <= 1e-3
            const double rho = ev == EV_ACCEPT ? std::nextafter(1e-3, 1.0) + (2.0 - std::nextafter(1e-3, 1.0)) * u(rng) : -u(rng);
            const bool fail_ref = parent_event(radius, decrease, invalid, ev, rho);
            bool fail = false;
            if (ev == EV_INVALID)
            {
                CHECK(!lm_trust::step_is_valid(0, -1.0), "a negative model cost change is invalid");
                fail = tr.on_invalid();
            }
            else
            {
                tr.on_valid();
                CHECK(lm_trust::accepts(rho) == (ev == EV_ACCEPT), "accepts(%g)", rho);
                if (lm_trust::accepts(rho))
                    tr.on_accept(rho);
                else
                    tr.on_reject();
            }
            events++;
            CHECK(fail == fail_ref, "sequence %d event %d: fail %d vs %d", seq, e, (int)fail, (int)fail_ref);
            CHECK(same_bits(tr.radius, radius) && same_bits(tr.decrease, decrease) && tr.invalid == invalid,
                  "sequence %d event %d (%d): radius %.17g vs %.17g, decrease %g vs %g, invalid %d vs %d", seq, e, ev, tr.radius, radius,
                  tr.decrease, decrease, tr.invalid, invalid);
            CHECK(tr.radius_exhausted() == (radius <= 1e-32), "radius floor at %g", radius);
            if (fail_ref)
                break;
        }
    }
    // the remaining decisions, against the parent's expressions
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(lm_trust::step_is_valid(0, 1e-300) && !lm_trust::step_is_valid(1, 1.0) && !lm_trust::step_is_valid(0, 0.0) &&
              !lm_trust::step_is_valid(0, nan) && !lm_trust::step_is_valid(0, inf),
          "step_is_valid");
    for (int i = 0; i < 10000; i++)
    {
        const double a = std::pow(10.0, -12.0 + 14.0 * u(rng)), b = std::pow(10.0, -3.0 + 6.0 * u(rng)), c = (u(rng) - 0.5) * a;
        CHECK(lm_trust::parameter_converged(a, b, 1e-8) == (a <= 1e-8 * (b + 1e-8)), "parameter tolerance");
        CHECK(lm_trust::function_converged(c, b, 1e-6) == (std::abs(c) <= 1e-6 * b), "function tolerance");
    }
    CHECK(!lm_trust::parameter_converged(nan, 1.0, 1e-8) && !lm_trust::function_converged(nan, 1.0, 1e-6) && !lm_trust::accepts(nan),
          "NaN decides nothing");
    {
        // a NaN rho that were accepted: 1/3 from the max, so the radius triples; a NaN radius becomes the cap
        lm_trust tr;
        tr.start(1.0);
        double radius = 1.0, decrease = 2.0;
        const double t = 2.0 * nan - 1.0;
        radius = radius / std::max(1.0 / 3.0, 1.0 - t * t * t);
        radius = std::min(1e16, radius);
        tr.on_accept(nan);
        CHECK(same_bits(tr.radius, radius) && same_bits(tr.decrease, decrease), "on_accept(NaN): %g vs %g", tr.radius, radius);
        tr.radius = nan;
        tr.on_accept(0.5);
        CHECK(same_bits(tr.radius, std::min(1e16, nan)), "a NaN radius: %g", tr.radius);
    }
    printf("trust: %ld events\n", events);
}
} // namespace

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "quat_plus")
        test_quat_plus();
    else if (what == "quat_normalize")
        test_quat_normalize();
    else if (what == "diagonal")
        test_diagonal();
    else if (what == "trust")
        test_trust();
    else
    {
        printf("usage: lm_rules_driver quat_plus | quat_normalize | diagonal | trust\n");
        return 2;
    }
    if (failures)
    {
        printf("FAIL %d checks\n", failures);
        return 1;
    }
    printf("ok %s\n", what.c_str());
    return 0;
}
