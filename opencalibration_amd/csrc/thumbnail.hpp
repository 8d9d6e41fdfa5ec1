// The rules of the load stage's image thumbnail (reference: src/extract/extract_image.cpp:42-52), shared by the device
// route (thumbnail.hip, hipcc) and the CPU route (host/thumbnail.cpp, g++):
//
//     cvtColor(image, lab, COLOR_BGR2Lab); scale = 50 / sqrt(area); resize(lab, thumb_lab, Size(0, 0), scale, scale, INTER_AREA);
//     cvtColor(thumb_lab, thumb, COLOR_Lab2BGR); thumbnail = R, G, B layers
//
// Both routes are built with -ffp-contract=off and use only correctly rounded operations here, so they agree to the bit.
// The colour is ortho_layers.hpp's (departure L1); the resize is cv::resize's INTER_AREA: its general
// path with the taps of area_table.hpp, or - when 1 / scale is an integer n to within DBL_EPSILON - ResizeAreaFast's
// integer cells.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "ortho_layers.hpp"

namespace ochip_th
{

struct plan
{
    int32_t rows, cols; // the thumbnail's size
    int32_t n;          // > 0: the integer path with n x n cells; 0: the general path
    double inv_scale;   // cv::resize's scale_x = scale_y = 1 / scale, the argument of area_table
};

enum
{
    SIZE_OK = 0,
    SIZE_BAD = 1,   // a side outside 1..65535
    SIZE_SMALL = 2, // fewer than 2 500 pixels: scale > 1, where INTER_AREA is a bilinear variant that is not restated
    SIZE_EMPTY = 3  // a side of the thumbnail rounds to 0
};

// host only (called once per batch): cv::resize's dsize = saturate_cast<int>(ssize * scale), rint with ties to even
inline int make_plan(int width, int height, plan *p)
{
    if (width < 1 || height < 1 || width > 65535 || height > 65535)
        return SIZE_BAD;
    const int64_t area = (int64_t)width * height;
    if (area < 2500)
        return SIZE_SMALL;
    const double scale = 50.0 / std::sqrt((double)area);
    p->cols = (int32_t)std::rint(width * scale);
    p->rows = (int32_t)std::rint(height * scale);
    if (p->cols < 1 || p->rows < 1)
        return SIZE_EMPTY;
    p->inv_scale = 1.0 / scale;
    const int n = (int)std::rint(p->inv_scale);
    p->n = std::fabs(p->inv_scale - n) < DBL_EPSILON ? n : 0;
    return SIZE_OK;
}

inline const char *size_error(int code)
{
    return code == SIZE_BAD     ? "an image side outside 1..65535"
           : code == SIZE_SMALL ? "an image of fewer than 2500 pixels has no thumbnail (its scale would exceed 1)"
                                : "a side of the thumbnail rounds to 0";
}

// a pixel's 8-bit Lab as one word: L | a << 8 | b << 16 (an entry of the device's table of all 2^24 BGR codes)
OCHIP_OL uint32_t lab_word(const ochip_ol::lab_tables &T, uint32_t bgr_code)
{
    const uint8_t bgr[3] = {(uint8_t)bgr_code, (uint8_t)(bgr_code >> 8), (uint8_t)(bgr_code >> 16)};
    uint8_t lab[3];
    ochip_ol::lab8_from_bgr8(T, bgr, lab);
    return (uint32_t)lab[0] | (uint32_t)lab[1] << 8 | (uint32_t)lab[2] << 16;
}

// saturate_cast<uchar>(float): cvRound, then the clamp
OCHIP_OL uint8_t round8(float v)
{
    const float r = rintf(v);
    return r <= 0.0f ? 0 : r >= 255.0f ? 255 : (uint8_t)r;
}

// general path: one tap of either chain, buf += S * alpha then sum += buf * beta
OCHIP_OL float tap(float acc, float value, float weight)
{
    return acc + value * weight;
}

// the source range [*first, *first + *count) of integer cell d along an axis of `size` pixels
OCHIP_OL void cell_range(int d, int n, int size, int *first, int *count)
{
    *first = d * n;
    *count = size - *first < n ? size - *first : n;
}

// integer path: the sum of a cell's in-range codes -> the code.  A complete cell (nx == ny == n) scales by the float
// 1 / (n * n); a partial one - a bottom row of cells that leaves the image, a column past width / n - divides by its count
OCHIP_OL uint8_t cell_value(uint32_t sum, int nx, int ny, int n)
{
    if (nx == n && ny == n)
        return round8((float)sum * (1.0f / (float)(n * n)));
    return round8((float)sum / (float)(nx * ny));
}

// the thumbnail's pixel from its resized 8-bit Lab: COLOR_Lab2BGR, then the R, G, B order of RasterToRGB
OCHIP_OL void rgb_from_lab8(const ochip_ol::lab_tables &T, const uint8_t lab[3], uint8_t rgb[3])
{
    uint8_t bgr[3];
    ochip_ol::bgr8_from_lab8(T, lab, bgr);
    rgb[0] = bgr[2], rgb[1] = bgr[1], rgb[2] = bgr[0];
}

} // namespace ochip_th
