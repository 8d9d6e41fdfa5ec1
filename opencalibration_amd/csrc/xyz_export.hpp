// The point cloud file of the reference (toXYZ / filterOutliers, src/io/saveXYZ.cpp) as plain functions, for host loops and
// kernels alike: the integer cell of a coordinate, the outlier box of one axis, the box test and
// the bytes `ostream << double` writes at its default precision.  Integer arithmetic only; nothing here depends on the
// floating-point contraction mode.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

#if defined(__HIPCC__)
#define OCHIP_XE_HD __host__ __device__ inline
#else
#define OCHIP_XE_HD inline
#endif

namespace ochip_xe
{

constexpr int SLOT = 48;        // bytes of a point's line slot: three numbers of at most 13 characters, two commas, a newline
constexpr int NUMBER_CHARS = 16; // room format_g6 and the host formatter are given per number

// static_cast<int64_t>(p[i]) is defined for these and for no other value
OCHIP_XE_HD bool key_defined(double v)
{
    return v > -9223372036854775808.0 && v < 9223372036854775808.0; // false for a NaN
}

OCHIP_XE_HD int64_t axis_key(double v) // truncation toward zero: -0.9 and 0.9 share key 0
{
    return static_cast<int64_t>(v);
}

struct bounds3 // the box of toXYZ: per axis (first, second)
{
    int64_t lo[3], hi[3];
};

// toXYZ's test: a box whose three axes are all empty passes everything, else every axis strictly inside
OCHIP_XE_HD bool filter_is_off(const bounds3 &b)
{
    return b.lo[0] == b.hi[0] && b.lo[1] == b.hi[1] && b.lo[2] == b.hi[2];
}

OCHIP_XE_HD bool inbounds(const bounds3 &b, double x, double y, double z)
{
    if (filter_is_off(b))
        return true;
    bool res = true;
    res &= (double)b.lo[0] < x && x < (double)b.hi[0];
    res &= (double)b.lo[1] < y && y < (double)b.hi[1];
    res &= (double)b.lo[2] < z && z < (double)b.hi[2];
    return res;
}

// filterOutliers' box of one axis from its (key, count) rows in ascending key order and the number of points
inline std::pair<int64_t, int64_t> dimbox(const int64_t *keys, const uint64_t *counts, size_t rows, size_t total)
{
    if (rows == 0)
        return {0, 0};
    const size_t cutoff = total * 0.025;
    size_t lowSum = 0, lowIndex = 0;
    while (lowIndex < rows && lowSum < cutoff)
        lowSum += counts[lowIndex++];
    if (lowIndex > 0)
        lowIndex--;
    size_t highSum = 0, highIndex = rows - 1;
    while (highIndex > lowIndex && highSum < cutoff)
        highSum += counts[highIndex--];
    const int64_t lowBound = keys[lowIndex], highBound = keys[highIndex];
    // (two's complement arithmetic where the reference's signed expressions overflow: keys further than 2^61 apart)
    const int64_t width = (int64_t)(((uint64_t)highBound - (uint64_t)lowBound) * 2u);
    const int64_t mid = (int64_t)((uint64_t)lowBound + (uint64_t)(width / 2));
    return {(int64_t)((uint64_t)mid - (uint64_t)width), (int64_t)((uint64_t)mid + (uint64_t)width)};
}

OCHIP_XE_HD uint64_t pow10_u64(int k) // 10^k, k in 0 .. 19
{
    uint64_t p = 1;
    for (int i = 0; i < k; i++)
        p *= 10u;
    return p;
}

OCHIP_XE_HD uint64_t double_bits(double v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(v);
#else
    union
    {
        double d;
        uint64_t u;
    } c;
    c.d = v;
    return c.u;
#endif
}

// The bytes of `ostream << v` at the default precision - printf("%g"): six significant digits, round-half-even on the exact
// binary value, trailing zeros and a bare point dropped, scientific form when the decimal exponent after rounding is < -4
// or >= 6.  Exact for +-0 and 1e-5 <= |v| < 2^63; returns the length (1 .. 12), or 0 for any other value ("not mine": the
// caller formats that number with snprintf on the host).  No terminator is written.
OCHIP_XE_HD int format_g6(double v, char *out)
{
    const uint64_t bits = double_bits(v);
    const bool negative = (bits >> 63) != 0;
    const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
    const int biased = (int)(mag >> 52);
    // 0x3EE4F8B588E368F1 is the double 1e-5 (it lies above 10^-5); 1086 is the exponent of 2^63
    if (mag != 0 && (mag < 0x3EE4F8B588E368F1ull || biased >= 1086))
        return 0; // nothing written
    int len = 0;
    if (negative)
        out[len++] = '-';
    if (mag == 0)
    {
        out[len++] = '0';
        return len;
    }
    const uint64_t m = (mag & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull; // |v| = m 2^e, 2^52 <= m < 2^53
    const int e = biased - 1075, b = biased - 1023;                         // -69 <= e <= 10, -17 <= b <= 62
    // floor(b log10(2)) for |b| < 2^10; |v| lies in [2^b, 2^(b+1)), so its decimal exponent is this or one more
    int X = ((b * 1233) >> 12) + 1;
    uint64_t q = 0;
    int cmp = 0; // the remainder against one half: -1 below, 0 at, 1 above
    for (int attempt = 0; attempt < 2; attempt++, X--)
    {
        const int k = 5 - X; // q = floor(|v| 10^k)
        if (k >= 0)
        {
            // here |v| < 10^7 < 2^24, so e <= -29: m 10^k (k <= 11, below 2^90) shifted right by s = -e in 29 .. 69
            const unsigned __int128 p = (unsigned __int128)m * pow10_u64(k);
            const int s = -e;
            const unsigned __int128 rem = p & ((((unsigned __int128)1) << s) - 1), half = ((unsigned __int128)1) << (s - 1);
            q = (uint64_t)(p >> s);
            cmp = rem < half ? -1 : rem > half ? 1 : 0;
        }
        else
        {
            // |v| >= 10^5: m 2^e / 10^j with j = -k in 1 .. 14.  e >= 0: the integer m << e is below 2^63.  e < 0: the
            // divisor 10^j 2^s = m / |v| 10^j < 2^53 / 10^4
            const uint64_t p10 = pow10_u64(-k);
            const uint64_t num = e >= 0 ? m << e : m, den = e >= 0 ? p10 : p10 << -e;
            q = num / den;
            const uint64_t rem = num - q * den, rest = den - rem; // rem < half <=> rem < den - rem
            cmp = rem < rest ? -1 : rem > rest ? 1 : 0;
        }
        if (q >= 100000u)
            break; // q < 10^6 by the choice of the first X; else X was one too large
    }
    if (cmp > 0 || (cmp == 0 && (q & 1u)))
        q++;
    if (q == 1000000u)
        q = 100000u, X++;
    // the six digits as nibbles, the first digit highest: no per-thread array, a kernel keeps them in a register
    uint32_t r = (uint32_t)q, d = 0;
    for (int i = 0; i < 6; i++)
    {
        d |= (r % 10u) << (4 * i);
        r /= 10u;
    }
    int nd = 6; // digits left once the trailing zeros are dropped
    while (nd > 1 && ((d >> (4 * (6 - nd))) & 15u) == 0)
        nd--;
#define OCHIP_XE_DIGIT(i) ((char)('0' + (int)((d >> (4 * (5 - (i)))) & 15u)))
    if (X < -4 || X >= 6)
    {
        out[len++] = OCHIP_XE_DIGIT(0);
        if (nd > 1)
        {
            out[len++] = '.';
            for (int i = 1; i < nd; i++)
                out[len++] = OCHIP_XE_DIGIT(i);
        }
        out[len++] = 'e';
        out[len++] = X < 0 ? '-' : '+';
        const int ax = X < 0 ? -X : X; // at most 18
        out[len++] = (char)('0' + ax / 10);
        out[len++] = (char)('0' + ax % 10);
    }
    else if (X >= 0)
    {
        for (int i = 0; i <= X; i++)
            out[len++] = OCHIP_XE_DIGIT(i);
        if (nd > X + 1)
        {
            out[len++] = '.';
            for (int i = X + 1; i < nd; i++)
                out[len++] = OCHIP_XE_DIGIT(i);
        }
    }
    else
    {
        out[len++] = '0';
        out[len++] = '.';
        for (int i = -1; i > X; i--)
            out[len++] = '0';
        for (int i = 0; i < nd; i++)
            out[len++] = OCHIP_XE_DIGIT(i);
    }
#undef OCHIP_XE_DIGIT
    return len;
}

// One point's line "x,y,z\n" into its slot from three formatted numbers; returns its length (at most 3 * 13 + 3)
OCHIP_XE_HD int join_line(const char *x, int lx, const char *y, int ly, const char *z, int lz, char *line)
{
    int n = 0;
    for (int i = 0; i < lx; i++)
        line[n++] = x[i];
    line[n++] = ',';
    for (int i = 0; i < ly; i++)
        line[n++] = y[i];
    line[n++] = ',';
    for (int i = 0; i < lz; i++)
        line[n++] = z[i];
    line[n++] = '\n';
    return n;
}

} // namespace ochip_xe
