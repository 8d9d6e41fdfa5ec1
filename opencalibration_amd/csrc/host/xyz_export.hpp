// The point cloud file in host loops: csrc/xyz_export.hpp - the header the kernels of
// csrc/xyz_export.hip run - over a flat cloud xyz [n][3], under OpenMP.  filterOutliers and toXYZ of the reference
// (src/io/saveXYZ.cpp).  Header-only and free of the rest of the host library: the stand-alone sanitizer program
// (scripts/xyz_export_sanitize.cpp) builds from this file alone.
#pragma once

#include "../xyz_export.hpp"

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace opencalibration_amd
{
namespace xyz_host
{

// "%g" of any double into out (ochip_xe::NUMBER_CHARS bytes, no terminator needed by the caller): the integer formatter
// where it is exact, the C library for the rest (below 1e-5, from 2^63, subnormal, not finite)
inline int format_number(double v, char *out)
{
    const int l = ochip_xe::format_g6(v, out);
    return l ? l : std::snprintf(out, ochip_xe::NUMBER_CHARS, "%g", v);
}

// filterOutliers: bounds6 = {x first, x second, y first, ...}.  False and a message for a coordinate without an integer cell.
inline bool outlier_bounds(const double *xyz, size_t n, int64_t *bounds6, std::string *error)
{
    std::map<int64_t, uint64_t> rows[3];
    bool bad = false;
#pragma omp parallel
    {
        std::map<int64_t, uint64_t> mine[3]; // a real cloud has few cells per axis
        bool mine_bad = false;
#pragma omp for schedule(static) nowait
        for (size_t i = 0; i < n; i++)
            for (int a = 0; a < 3; a++)
            {
                const double v = xyz[3 * i + a];
                if (!ochip_xe::key_defined(v))
                    mine_bad = true;
                else
                    mine[a][ochip_xe::axis_key(v)]++;
            }
#pragma omp critical(ochip_xyz_outlier_bounds)
        {
            bad = bad || mine_bad;
            for (int a = 0; a < 3; a++)
                for (const auto &kc : mine[a])
                    rows[a][kc.first] += kc.second;
        }
    }
    if (bad)
    {
        if (error)
            *error = "a coordinate is not finite or not below 2^63 in magnitude";
        return false;
    }
    for (int a = 0; a < 3; a++)
    {
        std::vector<int64_t> keys;
        std::vector<uint64_t> counts;
        for (const auto &kc : rows[a])
            keys.push_back(kc.first), counts.push_back(kc.second);
        const std::pair<int64_t, int64_t> box = ochip_xe::dimbox(keys.data(), counts.data(), keys.size(), n);
        bounds6[2 * a] = box.first, bounds6[2 * a + 1] = box.second;
    }
    return true;
}

// toXYZ in two steps, as the device route: every point's line into its slot and its length (independent, in parallel), a
// serial prefix over the lengths for the order, then the lines copied to their offsets.
struct CloudText
{
    std::vector<char> slots;       // [n][SLOT]
    std::vector<uint8_t> len;      // [n], 0: the point is outside the box
    std::vector<uint64_t> offset;  // [n]
    uint64_t bytes = 0, kept = 0;

    void prepare(const double *xyz, size_t n, const int64_t *bounds6 /* or nullptr: no filter */)
    {
        ochip_xe::bounds3 box = {{0, 0, 0}, {0, 0, 0}};
        if (bounds6)
            for (int a = 0; a < 3; a++)
                box.lo[a] = bounds6[2 * a], box.hi[a] = bounds6[2 * a + 1];
        slots.assign(n * ochip_xe::SLOT, 0);
        len.assign(n, 0);
        offset.assign(n, 0);
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; i++)
        {
            const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
            if (!ochip_xe::inbounds(box, x, y, z))
                continue;
            char num[3][ochip_xe::NUMBER_CHARS];
            const int lx = format_number(x, num[0]), ly = format_number(y, num[1]), lz = format_number(z, num[2]);
            len[i] = (uint8_t)ochip_xe::join_line(num[0], lx, num[1], ly, num[2], lz, &slots[i * ochip_xe::SLOT]);
        }
        bytes = 0, kept = 0;
        for (size_t i = 0; i < n; i++)
        {
            offset[i] = bytes;
            bytes += len[i];
            kept += len[i] != 0;
        }
    }
    void fill(char *out) const // exactly `bytes` bytes
    {
        const size_t n = len.size();
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; i++)
            if (len[i])
                std::memcpy(out + offset[i], &slots[i * ochip_xe::SLOT], len[i]);
    }
};

} // namespace xyz_host
} // namespace opencalibration_amd
