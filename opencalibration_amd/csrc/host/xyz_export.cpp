// liboc_host.so: the deliverables the reference's runner writes after COMPLETE that are text - the filtered point cloud
// (filterOutliers + toXYZ, src/io/saveXYZ.cpp) and the textured OBJ with its MTL (generateTexturedOBJ,
// src/ortho/ortho.cpp:2125-2255).  The cloud goes through xyz_export.hpp in host loops (ctx == NULL) or through
// ochip_xyz_export_* on the device; the OBJ is host only.  DESIGN.md section 4.16.
#include "../../../include/oc_host.h"

#include "capi_graph.hpp"
#include "graph_io.hpp"
#include "xyz_export.hpp"

#include <cstdlib>
#include <fstream>

using namespace opencalibration_amd;

namespace
{

thread_local std::string g_error;

int fail(const std::string &why)
{
    g_error = why;
    return -1;
}

// all clouds of all surfaces, in surface, cloud, point order
std::vector<double> flatten(const och_surface *const *surfaces, size_t n_surfaces)
{
    size_t n = 0;
    for (size_t s = 0; s < n_surfaces; s++)
        for (const point_cloud &c : surfaces[s]->s.cloud)
            n += c.size();
    std::vector<double> xyz;
    xyz.reserve(3 * n);
    for (size_t s = 0; s < n_surfaces; s++)
        for (const point_cloud &c : surfaces[s]->s.cloud)
            for (const auto &p : c)
                xyz.insert(xyz.end(), p.begin(), p.end());
    return xyz;
}

struct device_export // an ochip_xyz_export for the length of a call
{
    ochip_xyz_export *e = nullptr;
    ~device_export()
    {
        ochip_xyz_export_destroy(e);
    }
};

int device_fail(ochip_ctx *ctx, const char *what)
{
    return fail(std::string(what) + ": " + ochip_last_error(ctx));
}

int bounds_of(const double *xyz, size_t n, ochip_ctx *ctx, int64_t *bounds6)
{
    if (!bounds6 || (n && !xyz))
        return fail("outlier bounds: NULL argument");
    if (!ctx)
    {
        std::string why;
        return xyz_host::outlier_bounds(xyz, n, bounds6, &why) ? 0 : fail("outlier bounds: " + why);
    }
    device_export d;
    if (ochip_xyz_export_create(ctx, xyz, n, &d.e) != OCHIP_OK)
        return device_fail(ctx, "ochip_xyz_export_create");
    if (ochip_xyz_export_bounds(d.e, bounds6) != OCHIP_OK)
        return device_fail(ctx, "ochip_xyz_export_bounds");
    return 0;
}

// malloc'd and NUL-terminated, as och_graph_to_json's
char *text_of(const double *xyz, size_t n, ochip_ctx *ctx, const int64_t *bounds6, size_t *len, uint64_t *kept)
{
    if (n && !xyz)
    {
        fail("cloud text: NULL argument");
        return nullptr;
    }
    char *buf = nullptr;
    uint64_t bytes = 0, lines = 0;
    if (!ctx)
    {
        xyz_host::CloudText t;
        t.prepare(xyz, n, bounds6);
        bytes = t.bytes, lines = t.kept;
        buf = (char *)std::malloc((size_t)bytes + 1);
        if (buf)
            t.fill(buf);
    }
    else
    {
        device_export d;
        if (ochip_xyz_export_create(ctx, xyz, n, &d.e) != OCHIP_OK)
        {
            device_fail(ctx, "ochip_xyz_export_create");
            return nullptr;
        }
        if (ochip_xyz_export_text_size(d.e, bounds6, &bytes, &lines) != OCHIP_OK)
        {
            device_fail(ctx, "ochip_xyz_export_text_size");
            return nullptr;
        }
        buf = (char *)std::malloc((size_t)bytes + 1);
        if (buf && ochip_xyz_export_text(d.e, buf, bytes) != OCHIP_OK)
        {
            std::free(buf);
            device_fail(ctx, "ochip_xyz_export_text");
            return nullptr;
        }
    }
    if (!buf)
    {
        fail("cloud text: out of memory");
        return nullptr;
    }
    buf[bytes] = '\0';
    if (len)
        *len = (size_t)bytes;
    if (kept)
        *kept = lines;
    return buf;
}

char *copy_out(const std::string &s, size_t *len)
{
    char *buf = (char *)std::malloc(s.size() + 1);
    if (!buf)
        return nullptr;
    std::memcpy(buf, s.data(), s.size());
    buf[s.size()] = '\0';
    if (len)
        *len = s.size();
    return buf;
}

void put(std::string &out, double v) // ostream << v
{
    char num[ochip_xe::NUMBER_CHARS];
    out.append(num, (size_t)xyz_host::format_number(v, num));
}

} // namespace

extern "C"
{

const char *och_export_last_error(void)
{
    return g_error.c_str();
}

int och_xyz_outlier_bounds(const double *xyz, size_t n, ochip_ctx *ctx, int64_t *bounds6)
{
    return bounds_of(xyz, n, ctx, bounds6);
}

char *och_xyz_to_text(const double *xyz, size_t n, ochip_ctx *ctx, const int64_t *bounds6, size_t *len, uint64_t *kept)
{
    return text_of(xyz, n, ctx, bounds6, len, kept);
}

int och_cloud_outlier_bounds(const och_surface *const *surfaces, size_t n_surfaces, ochip_ctx *ctx, int64_t *bounds6)
{
    if (n_surfaces && !surfaces)
        return fail("och_cloud_outlier_bounds: NULL argument");
    const std::vector<double> xyz = flatten(surfaces, n_surfaces);
    return bounds_of(xyz.data(), xyz.size() / 3, ctx, bounds6);
}

char *och_cloud_to_xyz(const och_surface *const *surfaces, size_t n_surfaces, ochip_ctx *ctx, const int64_t *bounds6, size_t *len,
                       uint64_t *kept)
{
    if (n_surfaces && !surfaces)
    {
        fail("och_cloud_to_xyz: NULL argument");
        return nullptr;
    }
    const std::vector<double> xyz = flatten(surfaces, n_surfaces);
    return text_of(xyz.data(), xyz.size() / 3, ctx, bounds6, len, kept);
}

int och_cloud_save_xyz(const och_surface *const *surfaces, size_t n_surfaces, ochip_ctx *ctx, const int64_t *bounds6, const char *path)
{
    if (!path)
        return fail("och_cloud_save_xyz: NULL path");
    size_t len = 0;
    char *text = och_cloud_to_xyz(surfaces, n_surfaces, ctx, bounds6, &len, nullptr);
    if (!text)
        return -1;
    std::ofstream out(path, std::ios::binary);
    const bool ok = out.is_open() && out.write(text, (std::streamsize)len) && out.flush();
    std::free(text);
    return ok ? 0 : fail(std::string("cannot write ") + path);
}

void och_format_g6(const double *values, size_t n, int with_fallback, char *text16, uint8_t *len)
{
    std::memset(text16, 0, n * ochip_xe::NUMBER_CHARS);
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++)
    {
        char *out = text16 + i * ochip_xe::NUMBER_CHARS;
        len[i] = (uint8_t)(with_fallback ? xyz_host::format_number(values[i], out) : ochip_xe::format_g6(values[i], out));
    }
}

int och_textured_obj(const och_surface *const *surfaces, size_t n_surfaces, int64_t width, int64_t height, double min_x, double max_y,
                     double gsd_x, double gsd_y, const char *mtl_name, const char *jpg_name, char **obj_out, size_t *obj_len,
                     char **mtl_out, size_t *mtl_len)
{
    if ((n_surfaces && !surfaces) || !mtl_name || !jpg_name || !obj_out || !mtl_out)
        return fail("och_textured_obj: NULL argument");
    *obj_out = *mtl_out = nullptr;
    std::string mtl = "newmtl orthomosaic_material\nKa 1.0 1.0 1.0\nKd 1.0 1.0 1.0\nKs 0.0 0.0 0.0\nmap_Kd ";
    mtl += jpg_name;
    mtl += "\n";

    std::string obj = "mtllib ";
    obj += mtl_name;
    obj += "\nusemtl orthomosaic_material\n";
    const double extent_x = width * gsd_x, extent_y = height * gsd_y;
    size_t global_vertex_offset = 0;
    for (size_t s = 0; s < n_surfaces; s++)
    {
        const MeshGraph &mesh = surfaces[s]->s.mesh;
        if (mesh.size_edges() == 0)
            continue;
        // node ids are insertion indices: ascending id is the array's order, the 1-based index id + 1 past the offset
        for (const MeshNode &node : mesh.nodes)
        {
            const double *loc = node.location;
            obj += "v ";
            put(obj, loc[0]), obj += ' ', put(obj, loc[1]), obj += ' ', put(obj, loc[2]);
            const double u = (loc[0] - min_x) / extent_x;
            const double v = 1.0 - (max_y - loc[1]) / extent_y;
            obj += "\nvt ";
            put(obj, u), obj += ' ', put(obj, v);
            obj += '\n';
        }
        for (const auto &face : mesh_faces(mesh)) // the PLY writer's faces in its order
        {
            obj += 'f';
            for (size_t corner : face)
            {
                const std::string index = std::to_string(global_vertex_offset + corner + 1);
                obj += ' ' + index + '/' + index;
            }
            obj += '\n';
        }
        global_vertex_offset += mesh.size_nodes();
    }
    *obj_out = copy_out(obj, obj_len);
    *mtl_out = copy_out(mtl, mtl_len);
    if (!*obj_out || !*mtl_out)
    {
        std::free(*obj_out), std::free(*mtl_out);
        *obj_out = *mtl_out = nullptr;
        return fail("och_textured_obj: out of memory");
    }
    return 0;
}

} // extern "C"
