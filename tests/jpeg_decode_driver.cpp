// The stand-alone program of test_jpeg_decode_host.py: the host route of the JPEG decoder (csrc/jpeg_decode.hpp run by
// host/jpeg_decode.cpp, compiled with OCHIP_JPEG_DECODE_STANDALONE) under -fsanitize=address,undefined.
// `jpeg_decode_driver list.txt`: every line of the list is "<file> <output> <apply orientation 0 / 1>"; the file's pixels
// go to <output> and one line "<status> <width> <height>" per file to the standard output.
#include "../include/oc_host.h"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    std::ifstream list(argv[1]);
    std::string in, out;
    int apply;
    och_jpeg_decoder *dec = nullptr;
    if (och_jpeg_decoder_create(nullptr, 0, &dec) != 0)
        return 3;
    const char *names[3] = {"ok", "unsupported", "corrupt"};
    while (list >> in >> out >> apply)
    {
        std::ifstream f(in, std::ios::binary);
        // exactly the file's bytes on the heap: a read past them is the sanitizer's to see
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        std::vector<uint8_t> exact(bytes.begin(), bytes.end());
        exact.shrink_to_fit();
        ochip_jpeg_file_info info;
        const uint8_t *none = reinterpret_cast<const uint8_t *>(&info);
        if (och_jpeg_info(exact.empty() ? none : exact.data(), exact.size(), apply, &info) != 0)
            return 4;
        std::vector<uint8_t> pixels(info.status == OCHIP_JPEG_OK ? (size_t)info.width * (size_t)info.height * 3 : 0);
        const uint8_t *files[1] = {exact.empty() ? none : exact.data()};
        const uint64_t sizes[1] = {exact.size()};
        if (och_jpeg_decoder_decode(dec, 1, files, sizes, apply, pixels.data(), pixels.size(), nullptr, &info, nullptr) != 0)
        {
            std::fprintf(stderr, "%s: %s\n", in.c_str(), och_jpeg_decode_last_error());
            return 5;
        }
        if (info.status < 0 || info.status > 2)
            return 6;
        if (info.status == OCHIP_JPEG_OK)
        {
            std::ofstream o(out, std::ios::binary);
            o.write(reinterpret_cast<const char *>(pixels.data()), (std::streamsize)pixels.size());
        }
        std::cout << names[info.status] << " " << info.width << " " << info.height << "\n";
    }
    och_jpeg_decoder_destroy(dec);
    och_jpeg_decoder_destroy(dec); // a dead handle is refused, not followed
    return 0;
}
