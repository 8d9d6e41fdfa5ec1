// liboc_host.so: C ABI of a survey's geo-referencing - image metadata (image_metadata.hpp), the local frame
// (geo_coord.hpp) and the GeoJSON camera graph (graph_io.hpp).  Host code only.
#include "../../../include/oc_host.h"

#include "capi_graph.hpp"
#include "geo_coord.hpp"
#include "graph_io.hpp"
#include "image_metadata.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <sstream>

using namespace opencalibration_amd;

struct och_geo
{
    GeoCoord coord;
};

extern "C"
{

int och_jpeg_metadata(const uint8_t *data, uint64_t size, double *numbers14, char *strings, uint64_t cap, uint64_t *needed)
{
    if (!data || !numbers14 || (!strings && cap))
        return -1;
    image_metadata m;
    const MetadataStatus status = extract_metadata(data, (size_t)size, m);
    const auto &cam = m.camera_info;
    const auto &cpt = m.capture_info;
    const std::string *texts[8] = {&cam.make, &cam.model, &cam.serial_no, &cam.lens_make, &cam.lens_model, &cpt.datum, &cpt.timestamp, &cpt.datestamp};
    uint64_t total = 0;
    for (const std::string *s : texts)
        total += std::strlen(s->c_str()) + 1; // up to a NUL inside: the fields are C strings on this side
    if (needed)
        *needed = total;
    if (total > cap)
        return -1;
    const double numbers[14] = {(double)cam.width_px, (double)cam.height_px, cam.focal_length_px, cam.principal_point_px[0], cam.principal_point_px[1],
                                cpt.latitude,         cpt.longitude,         cpt.altitude,        cpt.relativeAltitude,      cpt.rollDegree,
                                cpt.pitchDegree,      cpt.yawDegree,         cpt.accuracyXY,      cpt.accuracyZ};
    std::memcpy(numbers14, numbers, sizeof numbers);
    for (const std::string *s : texts)
    {
        const size_t k = std::strlen(s->c_str()) + 1;
        std::memcpy(strings, s->c_str(), k);
        strings += k;
    }
    return (int)status;
}

och_geo *och_geo_create(double latitude, double longitude)
{
    och_geo *geo = new och_geo();
    if (!geo->coord.setOrigin(latitude, longitude))
    {
        delete geo;
        return nullptr;
    }
    return geo;
}

void och_geo_destroy(och_geo *geo)
{
    delete geo;
}

void och_geo_origin(const och_geo *geo, double *origin4)
{
    origin4[0] = geo->coord.getOriginLatitude();
    origin4[1] = geo->coord.getOriginLongitude();
    origin4[2] = geo->coord.centreLatitude();
    origin4[3] = geo->coord.centreLongitude();
}

void och_geo_to_local(const och_geo *geo, size_t n, const double *lat_lon_alt, double *xyz)
{
    for (size_t i = 0; i < n; i++)
        geo->coord.toLocalCS(lat_lon_alt[3 * i], lat_lon_alt[3 * i + 1], lat_lon_alt[3 * i + 2], xyz + 3 * i);
}

void och_geo_to_wgs84(const och_geo *geo, size_t n, const double *xyz, double *lon_lat_alt)
{
    for (size_t i = 0; i < n; i++)
        geo->coord.toWGS84(xyz + 3 * i, lon_lat_alt + 3 * i);
}

size_t och_geo_wkt(const och_geo *geo, char *buf, size_t cap)
{
    const std::string wkt = geo->coord.getWKT();
    if (buf && cap > wkt.size())
        std::memcpy(buf, wkt.c_str(), wkt.size() + 1);
    return wkt.size();
}

char *och_graph_geojson(och_graph *g, const och_geo *geo, const uint64_t *node_ids, size_t n_nodes, const uint64_t *edge_ids, size_t n_edges,
                        size_t *len)
{
    std::vector<size_t> nodes, edges;
    if (node_ids)
        nodes.assign(node_ids, node_ids + n_nodes);
    else
    {
        for (const auto &node : g->graph.nodes())
            nodes.push_back(node.id);
        std::sort(nodes.begin(), nodes.end());
    }
    if (edge_ids)
        edges.assign(edge_ids, edge_ids + n_edges);
    else
    {
        for (const auto &edge : g->graph.edges())
            edges.push_back(edge.id);
        std::sort(edges.begin(), edges.end());
    }
    std::ostringstream out;
    const bool ok = visualizeGeoJson(
        g->graph, nodes, edges,
        [&](const double *local, double *global) {
            if (geo)
                geo->coord.toWGS84(local, global);
            else
                std::memcpy(global, local, 24);
        },
        out);
    if (!ok)
    {
        g->error = "geojson: an id that is not in the graph";
        return nullptr;
    }
    const std::string s = out.str();
    char *buf = (char *)std::malloc(s.size() + 1);
    if (!buf)
    {
        g->error = "geojson: out of memory";
        return nullptr;
    }
    std::memcpy(buf, s.data(), s.size());
    buf[s.size()] = '\0';
    if (len)
        *len = s.size();
    return buf;
}

} // extern "C"
