// Per-tile progress thumbnails of the layer and blend passes, DESIGN.md section 4.15: the reference hands its UI a TileUpdate
// per finished tile from generateLayeredGeoTIFF (src/ortho/ortho.cpp:1553-1614) and blendLayeredGeoTIFF (:1962-2011), each
// with a thumbnail of at most 128 x 128 of what the tile now looks like.  This header is the arithmetic for both routes: the
// tile and thumbnail geometry, the two pixel rules, the slot layout and the argument checks.  csrc/ortho_tile_thumbs.hip runs
// slot_value a lane per slot pixel, host/ortho_tile_thumbs.cpp in straight loops.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define OCHIP_TT_HD __host__ __device__ inline
#else
#define OCHIP_TT_HD inline
#endif

namespace ochip_tt
{

enum : int
{
    PASS_LAYERS = 1, // bgra [L][rows][cols][4] and weight [L][rows][cols], as ochip_ortho_layers writes them
    PASS_BLEND = 2   // rgba [rows][cols][4], as ochip_ortho_blend writes it
};
constexpr int32_t MAX_THUMB = 128;                // a thumbnail's longer side at most
constexpr int32_t MAX_TILE = 4096, MAX_LAYERS = 8; // as ochip_ortho_blend
constexpr uint32_t BACKGROUND_ALPHA = 255 * 20 / 100; // the reference's kBackgroundAlpha: 51

struct thumb_dims
{
    int32_t scale, w, h;
};

// the thumbnail of a tw x th tile: every scale-th pixel, the scale the smallest that brings the longer side to 128 or less
OCHIP_TT_HD thumb_dims dims_of(int32_t tw, int32_t th)
{
    const int32_t longer = tw > th ? tw : th;
    int32_t scale = (longer + (MAX_THUMB - 1)) / MAX_THUMB;
    scale = scale < 1 ? 1 : scale;
    return {scale, (tw + scale - 1) / scale, (th + scale - 1) / scale};
}

// tiles along a side of `size` pixels, and the extent of tile t (the last may be partial)
OCHIP_TT_HD int64_t tiles_along(int64_t size, int32_t T)
{
    return (size + T - 1) / T;
}
OCHIP_TT_HD int32_t tile_extent(int64_t size, int32_t T, int64_t t)
{
    const int64_t left = size - t * T;
    return (int32_t)(left < T ? left : T);
}
// a tile's slot in the output: slot_side^2 pixels of 4 bytes; the thumbnail lies densely at its start, the rest is zero
OCHIP_TT_HD int32_t slot_side(int32_t T)
{
    return T < MAX_THUMB ? T : MAX_THUMB;
}

// Pass 1, the pick among a pixel's layers in ascending order (bytes B, G, R, A as they lie in memory: B | G << 8 | R << 16 |
// A << 24).  A sample is valid exactly when its alpha > 0; a valid one whose weight is greater than the best so far (a float
// compare: a NaN never wins, an equal weight keeps the lower layer) becomes the best.  The pixel is (B, G, R, 255) when the
// best weight ends >= 0, else the background (0, 0, 0, 51) - also for a valid sample with a weight in (-1, 0), which raises
// the best weight and still ends below 0: the reference's expression as written.
struct layer_pick
{
    float best = -1.0f;
    uint32_t colour = 0;

    OCHIP_TT_HD void take(uint32_t bgra, float weight)
    {
        if ((bgra >> 24) > 0 && weight > best)
        {
            best = weight;
            colour = bgra & 0x00FFFFFFu;
        }
    }
    OCHIP_TT_HD uint32_t pixel() const
    {
        return best >= 0.0f ? (colour | 0xFF000000u) : (BACKGROUND_ALPHA << 24);
    }
};

// Pass 2: alpha > 0 gives (rgba[2], rgba[1], rgba[0], 255), else (0, 0, 0, 0) - the checkerboard the blend paints where no
// layer is valid has alpha 0 and comes out as zeros.
OCHIP_TT_HD uint32_t blend_pixel(uint32_t rgba)
{
    if ((rgba >> 24) == 0)
        return 0u;
    return (rgba >> 16 & 255u) | (rgba & 0x0000FF00u) | (rgba & 255u) << 16 | 0xFF000000u;
}

// One band: whole tile rows from its first row, `rows` rows of `cols` pixels (the last tile row and column may be partial).
struct band
{
    int32_t pass, cols, T, L;
    int64_t rows;
    const uint32_t *pixels; // pass 1: [L][rows][cols], pass 2: [rows][cols]
    const float *weight;    // pass 1: [L][rows][cols]

    OCHIP_TT_HD int64_t tiles_x() const
    {
        return tiles_along(cols, T);
    }
    OCHIP_TT_HD int64_t tiles() const
    {
        return tiles_x() * tiles_along(rows, T);
    }
    OCHIP_TT_HD size_t slot_pixels() const
    {
        return (size_t)slot_side(T) * (size_t)slot_side(T);
    }
};

// Pixel i of tile `tile`'s slot (tiles row-major over the band): thumbnail pixel (i / thumb_w, i % thumb_w) while i lies
// inside the thumbnail - it reads tile pixel (min(y scale, th - 1), min(x scale, tw - 1)) - and zero behind it.
OCHIP_TT_HD uint32_t slot_value(const band &B, int64_t tile, uint32_t i)
{
    const int64_t tx = tile % B.tiles_x(), ty = tile / B.tiles_x();
    const int32_t tw = tile_extent(B.cols, B.T, tx), th = tile_extent(B.rows, B.T, ty);
    const thumb_dims d = dims_of(tw, th);
    if (i >= (uint32_t)d.w * (uint32_t)d.h)
        return 0u;
    const int32_t y = (int32_t)(i / (uint32_t)d.w), x = (int32_t)(i % (uint32_t)d.w);
    const int32_t r = y * d.scale < th - 1 ? y * d.scale : th - 1, c = x * d.scale < tw - 1 ? x * d.scale : tw - 1;
    const size_t at = (size_t)(ty * B.T + r) * (size_t)B.cols + (size_t)(tx * B.T + c);
    if (B.pass == PASS_BLEND)
        return blend_pixel(B.pixels[at]);
    const size_t plane = (size_t)B.rows * (size_t)B.cols;
    layer_pick p;
    for (int32_t l = 0; l < B.L; l++)
        p.take(B.pixels[(size_t)l * plane + at], B.weight[(size_t)l * plane + at]);
    return p.pixel();
}

// Why a call is refused ("" when it is not): every route checks with this before it reads anything.
inline std::string refusal(int pass, int64_t cols, int64_t rows, int64_t tile_size, int64_t num_layers, const void *pixels,
                           const void *weight)
{
    if (pass != PASS_LAYERS && pass != PASS_BLEND)
        return "pass " + std::to_string(pass) + " is neither 1 (layers) nor 2 (blend)";
    if (tile_size < 1 || tile_size > MAX_TILE)
        return "tile_size " + std::to_string(tile_size) + " outside 1.." + std::to_string(MAX_TILE);
    if (num_layers < 1 || num_layers > MAX_LAYERS)
        return "num_layers " + std::to_string(num_layers) + " outside 1.." + std::to_string(MAX_LAYERS);
    if (cols <= 0 || rows <= 0 || cols > 0x7FFFFFFF)
        return "a band of " + std::to_string(cols) + " x " + std::to_string(rows) + " pixels";
    if (!pixels)
        return "the pixels are NULL";
    if (pass == PASS_LAYERS && !weight)
        return "pass 1 needs the layers' weights";
    if ((uintptr_t)pixels % 4 || (uintptr_t)weight % 4)
        return "the arrays are not 4-byte aligned";
    if (tiles_along(cols, (int32_t)tile_size) * tiles_along(rows, (int32_t)tile_size) > 0x7FFFFFFF)
        return "more than 2^31 - 1 tiles in one band";
    return "";
}

// The CPU route: every slot of the band in tile order, out [tiles][slot_side^2] pixels.
inline void cpu_route(const band &B, uint32_t *out)
{
    const int64_t n = B.tiles();
    const size_t slot = B.slot_pixels();
    for (int64_t tile = 0; tile < n; tile++)
        for (size_t i = 0; i < slot; i++)
            out[(size_t)tile * slot + i] = slot_value(B, tile, (uint32_t)i);
}

} // namespace ochip_tt
