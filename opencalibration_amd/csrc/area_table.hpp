// cv::resize's INTER_AREA decimation table, host only: shared by the extraction's downscale (akaze.hip) and the thumbnail
// pass (thumbnail.hip, host/thumbnail.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

struct area_tab
{
    std::vector<int> off, si;
    std::vector<float> alpha;
};
// cv::resize INTER_AREA decimation table (computeResizeAreaTab).  `scale` is cv::resize's own scale_x = 1. / inv_scale_x - with
// inv_scale_x the fx it was called with (extract_features passes the FLOAT 1600 / max side as a double: 1 / 0.4000000059604645 is
// not 2.5, and the taps' weights differ in their last bits) or dsize / ssize when it was given a size
inline area_tab area_table(int ssize, int dsize, double scale)
{
    area_tab t;
    for (int dx = 0; dx < dsize; dx++)
    {
        t.off.push_back((int)t.si.size());
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3)
        {
            t.si.push_back(sx1 - 1);
            t.alpha.push_back((float)((sx1 - fsx1) / cell));
        }
        for (int sx = sx1; sx < sx2; sx++)
        {
            t.si.push_back(sx);
            t.alpha.push_back((float)(1.0 / cell));
        }
        if (fsx2 - sx2 > 1e-3)
        {
            t.si.push_back(sx2);
            t.alpha.push_back((float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell));
        }
    }
    t.off.push_back((int)t.si.size());
    return t;
}
