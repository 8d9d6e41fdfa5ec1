// ORACLE — test infrastructure only (see oracle.hpp).
// Forward-mode dual numbers restating ceres::Jet<T,N> (ceres/jet.h) [3P]: value + N partials,
// with the same derivative formulas.  Used by the restated TinySolver autodiff and relax functors.
// S is the scalar: double (the reference's own), or long double for the high-precision evaluation of
// relax_eval.cpp.  A scalar operand of a mixed Jet / scalar operator is of type S (a double converts).
#pragma once

#include <cmath>

namespace oracle
{

template <int N, typename S = double> struct Jet
{
    using scalar = S;
    S a = 0;
    S v[N];
    Jet()
    {
        for (int i = 0; i < N; i++)
            v[i] = 0;
    }
    Jet(S s) : a(s) // NOLINT: implicit like ceres::Jet(const T&)
    {
        for (int i = 0; i < N; i++)
            v[i] = 0;
    }
    Jet(S s, int k) : a(s)
    {
        for (int i = 0; i < N; i++)
            v[i] = 0;
        v[k] = S(1.0);
    }
};

template <int N, typename S> inline Jet<N, S> operator+(const Jet<N, S> &f, const Jet<N, S> &g)
{
    Jet<N, S> h;
    h.a = f.a + g.a;
    for (int i = 0; i < N; i++)
        h.v[i] = f.v[i] + g.v[i];
    return h;
}
template <int N, typename S> inline Jet<N, S> operator-(const Jet<N, S> &f, const Jet<N, S> &g)
{
    Jet<N, S> h;
    h.a = f.a - g.a;
    for (int i = 0; i < N; i++)
        h.v[i] = f.v[i] - g.v[i];
    return h;
}
template <int N, typename S> inline Jet<N, S> operator-(const Jet<N, S> &f)
{
    Jet<N, S> h;
    h.a = -f.a;
    for (int i = 0; i < N; i++)
        h.v[i] = -f.v[i];
    return h;
}
template <int N, typename S> inline Jet<N, S> operator*(const Jet<N, S> &f, const Jet<N, S> &g)
{
    Jet<N, S> h;
    h.a = f.a * g.a;
    for (int i = 0; i < N; i++)
        h.v[i] = f.a * g.v[i] + f.v[i] * g.a;
    return h;
}
template <int N, typename S> inline Jet<N, S> operator/(const Jet<N, S> &f, const Jet<N, S> &g)
{
    // ceres: g_a_inverse = 1/g.a; f_a_by_g_a = f.a * g_a_inverse; v = (f.v - f_a_by_g_a * g.v) * g_a_inverse
    Jet<N, S> h;
    const S ginv = S(1.0) / g.a;
    const S fg = f.a * ginv;
    h.a = fg;
    for (int i = 0; i < N; i++)
        h.v[i] = (f.v[i] - fg * g.v[i]) * ginv;
    return h;
}
template <int N, typename S> inline Jet<N, S> operator+(const Jet<N, S> &f, typename Jet<N, S>::scalar s)
{
    Jet<N, S> h = f;
    h.a = f.a + s;
    return h;
}
template <int N, typename S> inline Jet<N, S> operator+(typename Jet<N, S>::scalar s, const Jet<N, S> &f)
{
    return f + s;
}
template <int N, typename S> inline Jet<N, S> operator-(const Jet<N, S> &f, typename Jet<N, S>::scalar s)
{
    Jet<N, S> h = f;
    h.a = f.a - s;
    return h;
}
template <int N, typename S> inline Jet<N, S> operator-(typename Jet<N, S>::scalar s, const Jet<N, S> &f)
{
    Jet<N, S> h;
    h.a = s - f.a;
    for (int i = 0; i < N; i++)
        h.v[i] = -f.v[i];
    return h;
}
template <int N, typename S> inline Jet<N, S> operator*(const Jet<N, S> &f, typename Jet<N, S>::scalar s)
{
    Jet<N, S> h;
    h.a = f.a * s;
    for (int i = 0; i < N; i++)
        h.v[i] = f.v[i] * s;
    return h;
}
template <int N, typename S> inline Jet<N, S> operator*(typename Jet<N, S>::scalar s, const Jet<N, S> &f)
{
    return f * s;
}
template <int N, typename S> inline Jet<N, S> operator/(const Jet<N, S> &f, typename Jet<N, S>::scalar s)
{
    const S sinv = S(1.0) / s;
    Jet<N, S> h;
    h.a = f.a * sinv;
    for (int i = 0; i < N; i++)
        h.v[i] = f.v[i] * sinv;
    return h;
}
template <int N, typename S> inline Jet<N, S> operator/(typename Jet<N, S>::scalar s, const Jet<N, S> &g)
{
    Jet<N, S> h;
    const S ginv = S(1.0) / g.a;
    h.a = s * ginv;
    const S m = -s / (g.a * g.a);
    for (int i = 0; i < N; i++)
        h.v[i] = g.v[i] * m;
    return h;
}
template <int N, typename S> inline Jet<N, S> &operator+=(Jet<N, S> &f, const Jet<N, S> &g)
{
    f = f + g;
    return f;
}
template <int N, typename S> inline Jet<N, S> &operator-=(Jet<N, S> &f, const Jet<N, S> &g)
{
    f = f - g;
    return f;
}
template <int N, typename S> inline Jet<N, S> &operator*=(Jet<N, S> &f, const Jet<N, S> &g)
{
    f = f * g;
    return f;
}
template <int N, typename S> inline Jet<N, S> &operator/=(Jet<N, S> &f, const Jet<N, S> &g)
{
    f = f / g;
    return f;
}
template <int N, typename S> inline Jet<N, S> &operator*=(Jet<N, S> &f, typename Jet<N, S>::scalar s)
{
    f = f * s;
    return f;
}
template <int N, typename S> inline Jet<N, S> &operator/=(Jet<N, S> &f, typename Jet<N, S>::scalar s)
{
    f = f / s;
    return f;
}

#define ORACLE_JET_CMP(op)                                                                                             \
    template <int N, typename S> inline bool operator op(const Jet<N, S> &f, const Jet<N, S> &g)                                         \
    {                                                                                                                  \
        return f.a op g.a;                                                                                             \
    }                                                                                                                  \
    template <int N, typename S> inline bool operator op(const Jet<N, S> &f, typename Jet<N, S>::scalar g)                                                \
    {                                                                                                                  \
        return f.a op g;                                                                                               \
    }                                                                                                                  \
    template <int N, typename S> inline bool operator op(typename Jet<N, S>::scalar f, const Jet<N, S> &g)                                                \
    {                                                                                                                  \
        return f op g.a;                                                                                               \
    }
ORACLE_JET_CMP(<)
ORACLE_JET_CMP(<=)
ORACLE_JET_CMP(>)
ORACLE_JET_CMP(>=)
ORACLE_JET_CMP(==)
ORACLE_JET_CMP(!=)
#undef ORACLE_JET_CMP

template <int N, typename S> inline Jet<N, S> scaled(const Jet<N, S> &f, S val, S dscale)
{
    Jet<N, S> h;
    h.a = val;
    for (int i = 0; i < N; i++)
        h.v[i] = dscale * f.v[i];
    return h;
}
template <int N, typename S> inline Jet<N, S> sqrt(const Jet<N, S> &f)
{
    const S t = std::sqrt(f.a);
    return scaled(f, t, S(1.0) / (S(2.0) * t));
}
template <int N, typename S> inline Jet<N, S> abs(const Jet<N, S> &f)
{
    // ceres: Jet(abs(f.a), copysign(1, f.a) * f.v)
    return scaled(f, std::abs(f.a), std::copysign(S(1.0), f.a));
}
template <int N, typename S> inline Jet<N, S> acos(const Jet<N, S> &f)
{
    return scaled(f, std::acos(f.a), S(-1.0) / std::sqrt(S(1.0) - f.a * f.a));
}
template <int N, typename S> inline Jet<N, S> asin(const Jet<N, S> &f)
{
    return scaled(f, std::asin(f.a), S(1.0) / std::sqrt(S(1.0) - f.a * f.a));
}
template <int N, typename S> inline Jet<N, S> sin(const Jet<N, S> &f)
{
    return scaled(f, std::sin(f.a), std::cos(f.a));
}
template <int N, typename S> inline Jet<N, S> cos(const Jet<N, S> &f)
{
    return scaled(f, std::cos(f.a), -std::sin(f.a));
}
template <int N, typename S> inline Jet<N, S> atan2(const Jet<N, S> &g, const Jet<N, S> &f)
{
    // ceres: tmp = 1/(f.a^2 + g.a^2); Jet(atan2(g.a, f.a), tmp * (-g.a * f.v + f.a * g.v))
    const S tmp = S(1.0) / (f.a * f.a + g.a * g.a);
    Jet<N, S> h;
    h.a = std::atan2(g.a, f.a);
    for (int i = 0; i < N; i++)
        h.v[i] = tmp * (-g.a * f.v[i] + f.a * g.v[i]);
    return h;
}
template <int N, typename S> inline bool isfinite(const Jet<N, S> &f)
{
    // ceres::isfinite(Jet): value and all partials finite
    if (!std::isfinite(f.a))
        return false;
    for (int i = 0; i < N; i++)
        if (!std::isfinite(f.v[i]))
            return false;
    return true;
}
template <int N, typename S> inline bool isnan(const Jet<N, S> &f)
{
    if (std::isnan(f.a))
        return true;
    for (int i = 0; i < N; i++)
        if (std::isnan(f.v[i]))
            return true;
    return false;
}
inline double value_of(double x)
{
    return x;
}
inline long double value_of(long double x)
{
    return x;
}
template <int N, typename S> inline S value_of(const Jet<N, S> &f)
{
    return f.a;
}

} // namespace oracle
