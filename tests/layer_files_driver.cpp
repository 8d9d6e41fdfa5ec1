// A stand-alone program over the host route of the layers and cameras GeoTIFF tiles (csrc/host/geotiff.cpp with
// csrc/deflate_rules.hpp), built by test_layer_files_host.py with the address and undefined-behaviour
// sanitizers.  The host route's source is compiled into this program; the device entries it would call with a context are
// stubs here, never reached because every writer is made with ctx NULL.  The raster and every band fed are heap blocks of
// exactly their size, and the streams are collected into blocks of exactly the size collect asks for, so a read or a write
// one byte out is seen.
// The reader's host route (csrc/host/geotiff_read.cpp built with OCHIP_GEOTIFF_READ_STANDALONE as a second source) runs here
// too, over good, damaged and truncated streams.
//   usage: layer_files_driver list.txt
//   a line "W <kind> <layers> <width> <height> <sparse> <step> <raster file> <streams file>": the layer-major raster fed in
//   bands of <step> rows; the streams go back to back into <streams file>; prints "<tiles> <bytes> <count> <count> ..."
//   a line "R <kind> <layers> <width> <height> <row0> <rows> <streams file> <offsets file> <raster file>": a row window through
//   och_geotiff_reader_read into a block of exactly layers x rows x width samples; prints "<bad tile>"
#include "../include/oc_host.h"

extern "C"
{
    const char *ochip_last_error(const ochip_ctx *)
    {
        return "no device route in this program";
    }
    int ochip_geotiff_create(ochip_ctx *, int, int64_t, int64_t, int, ochip_geotiff **)
    {
        return OCHIP_EINVAL;
    }
    int ochip_geotiff_create_layered(ochip_ctx *, int, int, int64_t, int64_t, int, ochip_geotiff **)
    {
        return OCHIP_EINVAL;
    }
    int ochip_geotiff_feed(ochip_geotiff *, int64_t, int64_t, const void *, int)
    {
        return OCHIP_EINVAL;
    }
    int ochip_geotiff_payloads(ochip_geotiff *, const uint8_t *, int64_t)
    {
        return OCHIP_EINVAL;
    }
    int ochip_geotiff_collect(ochip_geotiff *, uint8_t *, uint64_t, uint64_t *, uint64_t *, uint64_t, uint64_t *)
    {
        return OCHIP_EINVAL;
    }
    int ochip_geotiff_finish(ochip_geotiff *)
    {
        return OCHIP_EINVAL;
    }
    void ochip_geotiff_destroy(ochip_geotiff *)
    {
    }
}

#include "../opencalibration_amd/csrc/host/geotiff.cpp"

#include <fstream>
#include <iostream>
#include <sstream>

namespace
{
std::unique_ptr<uint8_t[]> exact_block(const std::string &path, size_t &n)
{
    std::ifstream f(path, std::ios::binary);
    std::vector<char> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    n = v.size();
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n)
        std::memcpy(p.get(), v.data(), n);
    return p;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    std::ifstream list(argv[1]);
    std::string line;
    och_geotiff *none = nullptr;
    if (och_geotiff_create_layered(nullptr, OCH_GEOTIFF_LAYERS8, OCH_GEOTIFF_MAX_LAYERS + 1, 4, 4, 1, &none) == 0 || none)
        return 3; // more layers than the tiles have room for: refused
    if (och_geotiff_create_layered(nullptr, OCH_GEOTIFF_RGBA8, 1, 4, 4, 1, &none) == 0 || none)
        return 3; // a kind without layers
    while (std::getline(list, line))
    {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "R")
        {
            int kind, layers;
            int64_t width, height, row0, rows;
            std::string spath, fpath, rpath;
            if (!(in >> kind >> layers >> width >> height >> row0 >> rows >> spath >> fpath >> rpath))
                return 4;
            och_geotiff_reader *r = nullptr;
            if (och_geotiff_reader_create_layered(nullptr, kind, layers, width, height, 512, 512, 2, 0, &r) != 0)
            {
                std::cout << "refused " << och_geotiff_read_last_error() << "\n";
                continue;
            }
            size_t ns = 0, nf = 0;
            const std::unique_ptr<uint8_t[]> streams = exact_block(spath, ns), raw = exact_block(fpath, nf);
            std::vector<uint64_t> offsets(nf / 8);
            if (nf)
                std::memcpy(offsets.data(), raw.get(), nf / 8 * 8);
            const size_t bytes = (size_t)layers * (size_t)rows * (size_t)width * (kind == OCH_GEOTIFF_CAMERAS32 ? 8 : 4);
            const std::unique_ptr<uint8_t[]> raster(new uint8_t[bytes]);
            int64_t bad = -1;
            if (och_geotiff_reader_read(r, (int64_t)offsets.size() - 1, streams.get(), offsets.data(), row0, rows, raster.get(), 0, &bad) != 0)
                std::cout << "refused " << och_geotiff_read_last_error() << "\n";
            else
            {
                if (bad < 0)
                    std::ofstream(rpath, std::ios::binary).write(reinterpret_cast<const char *>(raster.get()), (std::streamsize)bytes);
                std::cout << bad << "\n";
            }
            och_geotiff_reader_destroy(r);
            och_geotiff_reader_destroy(r); // a dead handle is refused, not followed
            continue;
        }
        if (what != "W")
            return 4;
        int kind, layers, sparse;
        int64_t width, height, step;
        std::string rpath, spath;
        if (!(in >> kind >> layers >> width >> height >> sparse >> step >> rpath >> spath))
            return 4;
        const size_t unit = kind == OCH_GEOTIFF_CAMERAS32 ? 8 : 4;
        size_t n = 0;
        const std::unique_ptr<uint8_t[]> raster = exact_block(rpath, n);
        if (n != (size_t)layers * (size_t)height * (size_t)width * unit || step < 1)
            return 5;
        och_geotiff *e = nullptr;
        if (och_geotiff_create_layered(nullptr, kind, layers, width, height, sparse, &e) != 0)
        {
            std::cout << "refused " << och_geotiff_last_error() << "\n";
            continue;
        }
        std::vector<uint8_t> all;
        std::vector<uint64_t> all_counts;
        const auto take = [&]() {
            uint64_t bytes = 0, tiles = 0;
            if (och_geotiff_collect(e, nullptr, 0, &bytes, nullptr, 0, &tiles) != 0)
                return false;
            const std::unique_ptr<uint8_t[]> buf(new uint8_t[bytes]);
            const std::unique_ptr<uint64_t[]> counts(new uint64_t[tiles]);
            if (och_geotiff_collect(e, buf.get(), bytes, &bytes, counts.get(), tiles, &tiles) != 0)
                return false;
            all.insert(all.end(), buf.get(), buf.get() + bytes);
            all_counts.insert(all_counts.end(), counts.get(), counts.get() + tiles);
            return true;
        };
        bool ok = true;
        const size_t row = (size_t)width * unit;
        for (int64_t r0 = 0; r0 < height && ok; r0 += step)
        {
            const int64_t rows = step < height - r0 ? step : height - r0;
            const std::unique_ptr<uint8_t[]> band(new uint8_t[(size_t)layers * (size_t)rows * row]); // [layers][rows][width]
            for (int l = 0; l < layers; l++)
                std::memcpy(band.get() + (size_t)l * (size_t)rows * row, raster.get() + ((size_t)l * (size_t)height + (size_t)r0) * row,
                            (size_t)rows * row);
            ok = och_geotiff_feed(e, r0, rows, band.get(), 0) == 0 && take();
        }
        ok = ok && och_geotiff_feed(e, height, 1, raster.get(), 0) != 0; // a row beyond the raster is refused, not copied
        ok = ok && och_geotiff_finish(e) == 0 && take();
        och_geotiff_destroy(e);
        och_geotiff_destroy(e); // a dead handle is refused, not followed
        if (!ok)
        {
            std::cout << "failed " << och_geotiff_last_error() << "\n";
            continue;
        }
        std::ofstream(spath, std::ios::binary).write(reinterpret_cast<const char *>(all.data()), (std::streamsize)all.size());
        std::cout << all_counts.size() << " " << all.size();
        for (const uint64_t c : all_counts)
            std::cout << " " << c;
        std::cout << "\n";
    }
    return 0;
}
