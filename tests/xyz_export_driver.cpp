// Yardstick of the point cloud and textured OBJ exports, written from the behaviour the exports
// promise and with none of the package's code: std::map for the per-axis cell counts, the outlier box's walk, and
// std::ostringstream << double for every number.  One thread, no tricks.
//
//   xyz_export_driver format IN OUT            IN: raw doubles; OUT: one `ostream << v` per line
//   xyz_export_driver cloud IN OUT MODE...     IN: raw doubles [n][3]; OUT: the cloud file; MODE: filter | none | six integers
//                                              stdout: "bounds x0 x1 y0 y1 z0 z1", "kept K" and "seconds BOX TEXT"
//   xyz_export_driver obj IN OBJ MTL           IN: a text scene (see read_scene); OBJ, MTL: the two texts
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

namespace
{

typedef std::pair<int64_t, int64_t> range;

std::vector<double> read_doubles(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<double> v(raw.size() / 8);
    if (!v.empty())
        std::memcpy(v.data(), raw.data(), v.size() * 8);
    return v;
}

// the box of one axis: rows sorted by cell; 2.5 % of the points may lie below the low cell and above the high one
range axis_box(const std::map<int64_t, size_t> &cells, size_t total)
{
    std::vector<std::pair<int64_t, size_t>> rows(cells.begin(), cells.end());
    if (rows.empty())
        return range(0, 0);
    const size_t cutoff = total * 0.025;
    size_t low_sum = 0, low = 0;
    while (low < rows.size() && low_sum < cutoff)
        low_sum += rows[low++].second;
    if (low > 0)
        low--;
    size_t high_sum = 0, high = rows.size() - 1;
    while (high > low && high_sum < cutoff)
        high_sum += rows[high--].second;
    const int64_t low_bound = rows[low].first, high_bound = rows[high].first;
    const int64_t width = (high_bound - low_bound) * 2;
    const int64_t mid = low_bound + width / 2;
    return range(mid - width, mid + width);
}

std::array<range, 3> outlier_box(const std::vector<double> &xyz)
{
    std::array<std::map<int64_t, size_t>, 3> cells;
    const size_t n = xyz.size() / 3;
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            cells[a][static_cast<int64_t>(xyz[3 * i + a])]++;
    return {axis_box(cells[0], n), axis_box(cells[1], n), axis_box(cells[2], n)};
}

size_t write_cloud(const std::vector<double> &xyz, const std::array<range, 3> &box, std::ostream &out)
{
    const bool everything = box[0].first == box[0].second && box[1].first == box[1].second && box[2].first == box[2].second;
    size_t kept = 0;
    std::ostringstream buffer;
    for (size_t i = 0; i < xyz.size() / 3; i++)
    {
        bool inside = true;
        for (int a = 0; a < 3 && !everything; a++)
        {
            const double v = xyz[3 * i + a];
            inside &= box[a].first < v && v < box[a].second;
        }
        if (!inside)
            continue;
        buffer << xyz[3 * i] << "," << xyz[3 * i + 1] << "," << xyz[3 * i + 2] << "\n";
        kept++;
    }
    out << buffer.str();
    return kept;
}

struct edge
{
    uint64_t source, dest, border, opposite[2];
};
struct surface
{
    std::vector<std::array<double, 3>> vertices;
    std::vector<edge> edges;
};
struct scene
{
    long width, height;
    double min_x, max_y, gsd_x, gsd_y;
    std::string mtl_name, jpg_name;
    std::vector<surface> surfaces;
};

// width height min_x max_y gsd_x gsd_y (doubles as %a) mtl jpg surfaces, then per surface: vertices edges, the vertices'
// x y z (%a), the edges' source dest border opposite0 opposite1 (an unset corner: 18446744073709551615)
bool read_scene(const char *path, scene &s)
{
    std::ifstream in(path);
    auto number = [&](double &d) {
        std::string w;
        in >> w;
        d = std::strtod(w.c_str(), nullptr);
    };
    size_t count = 0;
    in >> s.width >> s.height;
    number(s.min_x), number(s.max_y), number(s.gsd_x), number(s.gsd_y);
    in >> s.mtl_name >> s.jpg_name >> count;
    s.surfaces.resize(count);
    for (surface &f : s.surfaces)
    {
        size_t nv = 0, ne = 0;
        in >> nv >> ne;
        f.vertices.resize(nv), f.edges.resize(ne);
        for (auto &v : f.vertices)
            number(v[0]), number(v[1]), number(v[2]);
        for (edge &e : f.edges)
            in >> e.source >> e.dest >> e.border >> e.opposite[0] >> e.opposite[1];
    }
    return (bool)in;
}

void write_obj(const scene &s, std::ostream &obj, std::ostream &mtl)
{
    mtl << "newmtl orthomosaic_material\n"
        << "Ka 1.0 1.0 1.0\n"
        << "Kd 1.0 1.0 1.0\n"
        << "Ks 0.0 0.0 0.0\n"
        << "map_Kd " << s.jpg_name << "\n";
    obj << "mtllib " << s.mtl_name << "\n"
        << "usemtl orthomosaic_material\n";
    const double extent_x = s.width * s.gsd_x, extent_y = s.height * s.gsd_y;
    size_t before = 0; // vertices of the surfaces written so far
    for (const surface &f : s.surfaces)
    {
        if (f.edges.empty())
            continue;
        for (const auto &p : f.vertices) // ascending id
        {
            obj << "v " << p[0] << " " << p[1] << " " << p[2] << "\n";
            const double u = (p[0] - s.min_x) / extent_x;
            const double v = 1.0 - (s.max_y - p[1]) / extent_y;
            obj << "vt " << u << " " << v << "\n";
        }
        // a triangle per side of every edge: corners by ascending id, the first two exchanged when that order turns
        // clockwise (negative cross product), every triangle once, the list sorted
        std::vector<std::array<uint64_t, 3>> faces;
        for (const edge &e : f.edges)
            for (int side = 0; side < (e.border ? 1 : 2); side++)
            {
                const uint64_t third = e.opposite[side] == UINT64_MAX ? 0 : e.opposite[side];
                std::array<uint64_t, 3> t = {e.source, e.dest, third};
                std::sort(t.begin(), t.end());
                const auto &a = f.vertices[t[0]], &b = f.vertices[t[1]], &c = f.vertices[t[2]];
                if ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0)
                    std::swap(t[0], t[1]);
                if (std::find(faces.begin(), faces.end(), t) == faces.end())
                    faces.push_back(t);
            }
        std::sort(faces.begin(), faces.end());
        for (const auto &t : faces)
        {
            obj << "f";
            for (uint64_t corner : t)
                obj << " " << before + corner + 1 << "/" << before + corner + 1;
            obj << "\n";
        }
        before += f.vertices.size();
    }
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 4)
        return 2;
    const std::string mode = argv[1];
    if (mode == "format")
    {
        const std::vector<double> v = read_doubles(argv[2]);
        std::ostringstream text;
        for (double x : v)
            text << x << "\n";
        std::ofstream(argv[3], std::ios::binary) << text.str();
        return 0;
    }
    if (mode == "cloud" && argc >= 5)
    {
        const std::vector<double> xyz = read_doubles(argv[2]);
        std::array<range, 3> box = {range(0, 0), range(0, 0), range(0, 0)};
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = now();
        if (std::string(argv[4]) == "filter")
            box = outlier_box(xyz);
        else if (std::string(argv[4]) != "none")
        {
            if (argc < 10)
                return 2;
            for (int a = 0; a < 3; a++)
                box[a] = range(std::strtoll(argv[4 + 2 * a], nullptr, 10), std::strtoll(argv[5 + 2 * a], nullptr, 10));
        }
        const double t1 = now();
        std::ofstream out(argv[3], std::ios::binary);
        const size_t kept = write_cloud(xyz, box, out);
        out.flush();
        const double t2 = now();
        std::printf("bounds %lld %lld %lld %lld %lld %lld\nkept %zu\nseconds %.6f %.6f\n", (long long)box[0].first,
                    (long long)box[0].second, (long long)box[1].first, (long long)box[1].second, (long long)box[2].first,
                    (long long)box[2].second, kept, t1 - t0, t2 - t1);
        return 0;
    }
    if (mode == "obj" && argc >= 5)
    {
        scene s;
        if (!read_scene(argv[2], s))
            return 3;
        std::ofstream obj(argv[3], std::ios::binary), mtl(argv[4], std::ios::binary);
        write_obj(s, obj, mtl);
        return 0;
    }
    return 2;
}
