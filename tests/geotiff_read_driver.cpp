// A stand-alone program over the host route of the GeoTIFF reader (csrc/host/geotiff_read.cpp built with
// OCHIP_GEOTIFF_READ_STANDALONE, csrc/inflate_rules.hpp), built by test_geotiff_read_host.py with the address and
// undefined-behaviour sanitizers.  Every input is a heap block of exactly its size and every output a block of exactly the
// size the call is told, so a read or a write one byte out is seen.
//   usage: geotiff_read_driver list.txt
//   a line "I <stream file> <expect> <payload file>": one stream through och_geotiff_reader_inflate; prints "<status> <bytes>"
//   a line "R <samples> <is_float> <width> <height> <tile_w> <tile_h> <predictor> <row0> <rows> <streams file> <offsets file>
//           <raster file>": a row window through och_geotiff_reader_read; prints "<bad tile>"
#include "../include/oc_host.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

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

void write_block(const std::string &path, const uint8_t *p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(p), (std::streamsize)n);
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    std::ifstream list(argv[1]);
    std::string line;
    och_geotiff_reader *plain = nullptr;
    if (och_geotiff_reader_create(nullptr, 1, 0, 16, 16, 16, 16, 1, 0, &plain) != 0)
        return 3;
    while (std::getline(list, line))
    {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "I")
        {
            std::string zpath, opath;
            uint64_t expect = 0;
            in >> zpath >> expect >> opath;
            size_t n = 0;
            const std::unique_ptr<uint8_t[]> z = exact_block(zpath, n);
            const std::unique_ptr<uint8_t[]> out(new uint8_t[expect]);
            const uint64_t offsets[2] = {0, n};
            int32_t status = -1;
            uint64_t bytes = 0;
            if (och_geotiff_reader_inflate(plain, 1, z.get(), offsets, &expect, out.get(), expect, &status, &bytes) != 0)
            {
                std::cout << "refused " << och_geotiff_read_last_error() << "\n";
                continue;
            }
            if (status == 0)
                write_block(opath, out.get(), expect);
            std::cout << status << " " << bytes << "\n";
        }
        else if (kind == "R")
        {
            int samples, is_float, tw, th, predictor;
            int64_t width, height, row0, rows;
            std::string spath, fpath, rpath;
            in >> samples >> is_float >> width >> height >> tw >> th >> predictor >> row0 >> rows >> spath >> fpath >> rpath;
            och_geotiff_reader *r = nullptr;
            if (och_geotiff_reader_create(nullptr, samples, is_float, width, height, tw, th, predictor, 0, &r) != 0)
            {
                std::cout << "refused " << och_geotiff_read_last_error() << "\n";
                continue;
            }
            size_t ns = 0, nf = 0;
            const std::unique_ptr<uint8_t[]> streams = exact_block(spath, ns), raw = exact_block(fpath, nf);
            std::vector<uint64_t> offsets(nf / 8);
            if (nf)
                std::memcpy(offsets.data(), raw.get(), nf / 8 * 8);
            const size_t bytes = (size_t)rows * (size_t)width * (size_t)(is_float ? 4 : samples);
            const std::unique_ptr<uint8_t[]> raster(new uint8_t[bytes]);
            int64_t bad = -1;
            if (och_geotiff_reader_read(r, (int64_t)offsets.size() - 1, streams.get(), offsets.data(), row0, rows, raster.get(), 0, &bad) != 0)
                std::cout << "refused " << och_geotiff_read_last_error() << "\n";
            else
            {
                if (bad < 0)
                    write_block(rpath, raster.get(), bytes);
                std::cout << bad << "\n";
            }
            och_geotiff_reader_destroy(r);
            och_geotiff_reader_destroy(r); // a dead handle is refused, not followed
        }
        else
            return 4;
    }
    och_geotiff_reader_destroy(plain);
    return 0;
}
