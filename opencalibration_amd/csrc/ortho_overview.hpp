// Averaged overview levels of the orthomosaic (RGBA8) and the DSM (float32), DESIGN.md section 4.13: the reference ends every
// raster with BuildOverviews("AVERAGE", 2, 4, 8, ...) (src/ortho/ortho.cpp:944-961, 1642-1657, 2028-2044).  This header is the
// rule for both routes - the two cell functions, the level sizes - and the builder's bookkeeping: which rows of which level a
// band completes, as a list of steps that csrc/ortho_overview.hip runs as kernels and host/ortho_overview.cpp as loops.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define OCHIP_OV_HD __host__ __device__ inline
#else
#define OCHIP_OV_HD inline
#endif

namespace ochip_ov
{

enum : int
{
    KIND_RGBA8 = 0,  // 4 bytes a pixel, alpha last (BGRA alike: the colour channels are treated the same)
    KIND_FLOAT32 = 1 // NaN: no data
};
constexpr int FUSED_DEPTH = 6;               // the fused kernel's levels: a workgroup owns 64 x 64 pixels of level 0
constexpr int64_t FUSED_BLOCK = 1 << FUSED_DEPTH;
constexpr int MAX_LEVELS = 62;

// levels k = 1, 2, ... for every factor 2^k < min(width, height)
OCHIP_OV_HD int num_levels(int64_t width, int64_t height)
{
    const int64_t m = width < height ? width : height;
    int n = 0;
    while (n + 1 < MAX_LEVELS && ((int64_t)1 << (n + 1)) < m)
        n++;
    return n;
}
// columns or rows of level k of a side of `size` pixels: ceil(size / 2^k)
OCHIP_OV_HD int64_t level_extent(int64_t size, int k)
{
    return (size + (((int64_t)1 << k) - 1)) >> k;
}

// One RGBA8 pixel (R | G << 8 | B << 16 | A << 24 as the bytes lie in memory) from its cell of the level before: top-left a,
// top-right b, bottom-left c, bottom-right d; has_right / has_bottom: the cell's second column / row exists.  n counts the
// cell's pixels with alpha > 0, m all of them; a colour is (sum over the valid + n / 2) / n, alpha (sum over all + m / 2) / m.
OCHIP_OV_HD uint32_t rgba_cell(uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool has_right, bool has_bottom)
{
    const uint32_t px[4] = {a, b, c, d};
    const bool exists[4] = {true, has_right, has_bottom, has_right && has_bottom};
    uint32_t sum[4] = {0, 0, 0, 0}, n = 0, m = 0;
    for (int i = 0; i < 4; i++)
    {
        if (!exists[i])
            continue;
        m++;
        const uint32_t alpha = px[i] >> 24;
        sum[3] += alpha;
        if (alpha > 0)
        {
            n++;
            sum[0] += px[i] & 255u, sum[1] += px[i] >> 8 & 255u, sum[2] += px[i] >> 16 & 255u;
        }
    }
    if (n == 0)
        return 0u;
    return (sum[0] + n / 2) / n | (sum[1] + n / 2) / n << 8 | (sum[2] + n / 2) / n << 16 | (sum[3] + m / 2) / m << 24;
}

// One float32 pixel: the double sum of the cell's non-NaN pixels in the order a, b, c, d over their count, rounded once to
// float; NaN when there is none.  (x != x instead of isnan: the same test under every compiler setting.)
OCHIP_OV_HD float float_cell(float a, float b, float c, float d, bool has_right, bool has_bottom)
{
    const float px[4] = {a, b, c, d};
    const bool exists[4] = {true, has_right, has_bottom, has_right && has_bottom};
    double sum = 0.0;
    int n = 0;
    for (int i = 0; i < 4; i++)
        if (exists[i] && !(px[i] != px[i]))
            sum += (double)px[i], n++;
    if (n == 0)
    {
        union
        {
            uint32_t u;
            float f;
        } q;
        q.u = 0x7FC00000u;
        return q.f;
    }
    return (float)(sum / (double)n);
}

struct rgba_rule
{
    using type = uint32_t;
    static OCHIP_OV_HD uint32_t cell(uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool r, bool m)
    {
        return rgba_cell(a, b, c, d, r, m);
    }
};
struct float_rule
{
    using type = float;
    static OCHIP_OV_HD float cell(float a, float b, float c, float d, bool r, bool m)
    {
        return float_cell(a, b, c, d, r, m);
    }
};

// rows [r0, r1) of level `level` from the two source rows of each: a pixel (r, c) reads (2r .. 2r + 1, 2c .. 2c + 1) of the
// level before, `src` holding that level's rows from src_row0 on, src_w x src_h its whole size.  top (may be NULL): row 2 r0
// comes from there instead (the builder's pending row).  The CPU route's loop and the restatement of the plain kernel.
template <class R>
inline void level_rows(const typename R::type *src, int64_t src_row0, int64_t src_w, int64_t src_h, const typename R::type *top,
                       typename R::type *dst, int64_t dst_w, int64_t r0, int64_t r1)
{
#if defined(_OPENMP)
#pragma omp parallel for schedule(static)
#endif
    for (int64_t r = r0; r < r1; r++)
    {
        const bool has_bottom = 2 * r + 1 < src_h;
        const typename R::type *s0 = top && r == r0 ? top : src + (size_t)(2 * r - src_row0) * (size_t)src_w;
        const typename R::type *s1 = has_bottom ? src + (size_t)(2 * r + 1 - src_row0) * (size_t)src_w : s0;
        typename R::type *d = dst + (size_t)r * (size_t)dst_w;
        for (int64_t c = 0; c < dst_w; c++)
        {
            const bool has_right = 2 * c + 1 < src_w;
            const int64_t c1 = has_right ? 2 * c + 1 : 2 * c;
            d[c] = R::cell(s0[2 * c], s0[c1], s1[2 * c], s1[c1], has_right, has_bottom);
        }
    }
}

// ---- the builder's bookkeeping ---------------------------------------------------------------------------------------------
// One step of a feed.  PLAIN: rows [r0, r1) of `level` by the one-level rule, level 1 from the band (top_pending: row 2 r0 is
// the pending row kept from the feed before), levels >= 2 from the stored level before.  FUSED: level-0 rows [r0, r1) of the
// band, r0 a multiple of FUSED_BLOCK and r1 one too or the raster's height, through every level down to min(levels,
// FUSED_DEPTH) at once.  KEEP: the band's last row (level-0 row r0) becomes the pending row.
struct step
{
    enum what_t
    {
        PLAIN,
        FUSED,
        KEEP
    } what;
    int level;
    int64_t r0, r1;
    bool top_pending;
};

struct progress
{
    int64_t width = 0, height = 0;
    int levels = 0;
    int64_t fed = 0;                // level-0 rows fed so far
    bool finished = false;
    std::vector<int64_t> done;      // done[k], k = 1 .. levels: rows of level k computed ([0] unused)

    void reset(int64_t w, int64_t h)
    {
        width = w, height = h, levels = num_levels(w, h), fed = 0, finished = false;
        done.assign((size_t)levels + 1, 0);
    }
    int64_t level_w(int k) const
    {
        return level_extent(width, k);
    }
    int64_t level_h(int k) const
    {
        return level_extent(height, k);
    }
    // rows of level k that `have` complete rows of level k - 1 allow
    int64_t allowed(int k, int64_t have) const
    {
        return have == level_h(k - 1) ? level_h(k) : have / 2;
    }

    // Checks a feed and lists its steps; "" or the refusal.  fused: the fused kernel may take the aligned blocks.
    std::string feed(int64_t row0, int64_t rows, bool fused, std::vector<step> *steps)
    {
        steps->clear();
        auto span = [](int64_t a, int64_t b) { return "rows " + std::to_string(a) + " to " + std::to_string(b); };
        if (finished)
            return "feed of " + span(row0, row0 + rows) + " after finish";
        if (rows < 1 || row0 < 0)
            return "feed of " + std::to_string(rows) + " rows from row " + std::to_string(row0);
        if (row0 > fed)
            return "a gap: " + span(row0, row0 + rows) + " were fed, row " + std::to_string(fed) + " is next";
        if (row0 < fed)
            return "an overlap: " + span(row0, row0 + rows) + " were fed, row " + std::to_string(fed) + " is next";
        if (rows > height - row0)
            return span(row0, row0 + rows) + " were fed, the raster has " + std::to_string(height) + " rows";
        const int64_t end = row0 + rows;
        fed = end;
        if (levels == 0)
            return "";
        int64_t cur = row0;
        if (cur & 1) // the pending row and the band's first one
        {
            steps->push_back({step::PLAIN, 1, cur / 2, cur / 2 + 1, true});
            cur++;
        }
        // level-0 rows [cur, lim) pair up inside this band (the raster's last row may stand alone)
        const int64_t lim = end == height ? end : end & ~(int64_t)1;
        int64_t a = (cur + FUSED_BLOCK - 1) / FUSED_BLOCK * FUSED_BLOCK, b = a;
        if (fused && a < lim)
            b = end == height ? end : a + (lim - a) / FUSED_BLOCK * FUSED_BLOCK;
        if (b > a)
        {
            if (a > cur)
                steps->push_back({step::PLAIN, 1, cur / 2, a / 2, false});
            steps->push_back({step::FUSED, 1, a, b, false});
            if (lim > b)
                steps->push_back({step::PLAIN, 1, b / 2, (lim + 1) / 2, false});
        }
        else if (lim > cur)
            steps->push_back({step::PLAIN, 1, cur / 2, (lim + 1) / 2, false});
        if (lim < end)
            steps->push_back({step::KEEP, 0, end - 1, end, false});
        const int fd = levels < FUSED_DEPTH ? levels : FUSED_DEPTH;
        int64_t have = allowed(1, end);
        // levels the fused step wrote: what lies before its rows is done by the feeds before, what lies behind by the steps
        // of the level before (above); level 1 has its own steps
        done[1] = have;
        for (int k = 2; k <= levels; k++)
        {
            const int64_t to = allowed(k, have);
            int64_t from = done[k];
            if (b > a && k <= fd)
            {
                // rows [a >> k, ceil(b / 2^k)) come from the fused step
                const int64_t fa = a >> k, fb = b == height ? level_h(k) : b >> k;
                if (from < fa)
                    steps->push_back({step::PLAIN, k, from, fa, false});
                from = from > fb ? from : fb;
            }
            if (to > from)
                steps->push_back({step::PLAIN, k, from, to, false});
            done[k] = have = to;
        }
        return "";
    }
    std::string finish()
    {
        if (fed != height)
            return "finish before the last row: rows 0 to " + std::to_string(fed) + " of " + std::to_string(height) + " were fed";
        finished = true;
        return "";
    }
};

} // namespace ochip_ov
