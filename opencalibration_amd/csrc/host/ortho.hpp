// The orthomosaic preview and the DSM raster (src/ortho/ortho.cpp:228-472, 478-653, 793-964): the reference's context
// (bounds, GSD, involved nodes, output size clamps), a CPU route that restates its per-pixel loop with the mesh walker, and
// the device route (ortho.hip) over a triangle table built here.  GeoTIFF output, the layered full-resolution mosaic and
// everything that needs an image codec stay with the caller.
#pragma once

#include "relax_mesh.hpp"
#include "types.hpp"

#include "../../../include/ochip.h"

#include <string>
#include <vector>

namespace opencalibration_amd
{
namespace ortho
{

struct Bounds // OrthoMosaicBounds
{
    double min_x, max_x, min_y, max_y, mean_surface_z;
};

// OrthoMosaicContext without the k-d tree and the walkers: involved = indices (graph node order) of the nodes with a
// finite orientation
struct Context
{
    Bounds bounds;
    std::vector<size_t> involved;
    double gsd = 0, mean_camera_z = 0, average_camera_elevation = 0;
};

// the raster both outputs are rendered into
struct Plan
{
    int width = 0, height = 0;
    double gsd = 0;
    Bounds bounds{};
    double mean_camera_z = 0;
};

Bounds calculateBoundsAndMeanZ(const std::vector<const surface_model *> &surfaces);
// node_indices in the order the reference iterates its involved set
double calculateGSD(const MeasurementGraph &graph, const std::vector<size_t> &node_indices, double mean_surface_z, bool thumbnail);
Context prepareContext(const std::vector<const surface_model *> &surfaces, const MeasurementGraph &graph, bool thumbnail);
// input pixels = the involved nodes' model pixels_cols x pixels_rows (the reference reads metadata.camera_info, which the
// load stage copies into the model)
uint64_t inputPixels(const Context &context, const MeasurementGraph &graph);
void clampOutputResolution(double &gsd, int &width, int &height, uint64_t total_input_pixels);
void clampOutputMegapixels(double &gsd, int &width, int &height, double max_output_megapixels);
Plan thumbnailPlan(const Context &context, const MeasurementGraph &graph);
Plan dsmPlan(const Context &context, const MeasurementGraph &graph, double max_output_megapixels);

// every triangle of every surface, corners in ascending node order, surfaces in order; tri_off[s] .. tri_off[s + 1]
struct TriangleTable
{
    std::vector<uint64_t> tri_off{0};
    std::vector<double> tri9;
    std::vector<std::array<size_t, 3>> nodes; // the corners' node indices, ascending; sorted within a surface
};
TriangleTable triangleTable(const std::vector<const surface_model *> &surfaces);

// rayTraceHeight(x, y, mean_camera_z, surfaces) (ortho.cpp:462-472)
double rayTraceHeight(double x, double y, double mean_camera_z, const std::vector<const surface_model *> &surfaces);

// The CPU route of the height stage: rows [row0, row0 + rows) of the plan's raster, row-parallel, one walker per surface
// started afresh on every row (deterministic), reinitialised after a miss, first surface that hits wins; z in the
// triangle's canonical corner order (ortho_geom.hpp).  z [rows][width]; tri (may be NULL) the table index of the triangle.
// Returns the walks that ran out of steps (intersect.cpp:152-156).
uint64_t heightsCPU(const std::vector<const surface_model *> &surfaces, const Plan &plan, int64_t row0, int64_t rows,
                    double *z, uint32_t *tri, const TriangleTable *table);

// The preview's camera records (ochip_ortho_thumbnail's layout) of the involved nodes, their thumbnails concatenated.
// False + *error when an involved node has no thumbnail.
struct Cameras
{
    std::vector<double> cams24;
    std::vector<CameraModel> models; // the CPU route projects with these (image_from_3d)
    std::vector<uint32_t> ids;
    std::vector<uint64_t> thumb_off;
    std::vector<uint8_t> thumbs;
};
bool cameras(const Context &context, const MeasurementGraph &graph, Cameras *out, std::string *error);

// The CPU route of the preview's colour stage over heights z [height][width]: rgba [height][width][4], ids [height][width]
void colourCPU(const Plan &plan, const Cameras &cams, const double *z, uint8_t *rgba, uint32_t *ids);

} // namespace ortho
} // namespace opencalibration_amd
