// A stand-alone program over the host route of the decoder as och_ortho_stream_upload_jpegs drives it on the CPU route
// (opencalibration_amd/csrc/host/ortho_stream.cpp), for the sanitizers: the stream itself needs the
// graph, the mesh and the layered render and does not link alone, so this program makes the stream's calls of
// och_jpeg_decoder_decode - out the slot block, offsets[i] the planned slot's distance from its start, scattered and not
// ascending, two image sizes in one call - into a heap block of exactly capacity x slot_bytes, every file in a heap block of
// exactly its size.  Built by tests/test_ortho_stream_files_host.py from this file and host/jpeg_decode.cpp with
// -DOCHIP_JPEG_DECODE_STANDALONE -fsanitize=address,undefined; no Python, no preload.
//
//   ortho_stream_files_driver <list> <capacity> <slot_bytes> <out>
//
// <list>: one line per file, "<call> <slot> <width> <height> <path>", the calls ascending.  Before the calls two refusals
// are made and must leave the block untouched: a slot outside the block and a NULL file.  Prints "<call> <slot> <status>"
// per file and writes the block as it stands after the last call to <out>.  Exit status 1 when anything is not as the
// interface says.
#include "../include/oc_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace
{
struct entry
{
    int call = 0;
    uint64_t slot = 0;
    int width = 0, height = 0;
    uint8_t *data = nullptr; // a heap block of exactly size bytes
    uint64_t size = 0;
};

int bad(const std::string &what)
{
    std::fprintf(stderr, "ortho_stream_files_driver: %s\n", what.c_str());
    return 1;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 5)
        return bad("usage: <list> <capacity> <slot_bytes> <out>");
    const uint64_t capacity = std::strtoull(argv[2], nullptr, 10), slot_bytes = std::strtoull(argv[3], nullptr, 10);
    const uint64_t block_bytes = capacity * slot_bytes;
    std::vector<entry> entries;
    std::ifstream list(argv[1]);
    std::string line;
    while (std::getline(list, line))
    {
        std::istringstream in(line);
        entry e;
        std::string path;
        if (!(in >> e.call >> e.slot >> e.width >> e.height >> path))
            continue;
        std::ifstream f(path, std::ios::binary);
        const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (!f || bytes.empty())
            return bad("cannot read " + path);
        e.size = bytes.size();
        e.data = static_cast<uint8_t *>(std::malloc(bytes.size()));
        std::memcpy(e.data, bytes.data(), bytes.size());
        entries.push_back(e);
    }
    if (entries.size() < 2)
        return bad("the list names fewer than two files");
    uint8_t *block = static_cast<uint8_t *>(std::malloc(block_bytes));
    std::memset(block, 0xA5, block_bytes);
    och_jpeg_decoder *dec = nullptr;
    if (och_jpeg_decoder_create(nullptr, 0, &dec) != 0)
        return bad(och_jpeg_decode_last_error());
    static const char *const names[3] = {"ok", "unsupported", "corrupt"};
    int rc = 0;
    {
        // the refusals: nothing may be written
        const uint8_t *files[2] = {entries[0].data, entries[1].data};
        const uint64_t sizes[2] = {entries[0].size, entries[1].size};
        uint64_t offsets[2] = {0, block_bytes - 1};
        ochip_jpeg_file_info info[2];
        if (och_jpeg_decoder_decode(dec, 2, files, sizes, 1, block, block_bytes, offsets, info, nullptr) != -1)
            rc = bad("a slot outside the block was not refused");
        else
            std::printf("# refused: a slot outside the block\n");
        offsets[1] = slot_bytes;
        files[1] = nullptr;
        if (och_jpeg_decoder_decode(dec, 2, files, sizes, 1, block, block_bytes, offsets, info, nullptr) != -1)
            rc = bad("a NULL file was not refused");
        else
            std::printf("# refused: a NULL file\n");
        for (uint64_t i = 0; i < block_bytes; i++)
            if (block[i] != 0xA5)
            {
                rc = bad("a refused call wrote byte " + std::to_string(i));
                break;
            }
    }
    for (size_t a = 0; a < entries.size() && rc == 0;)
    {
        size_t b = a;
        while (b < entries.size() && entries[b].call == entries[a].call)
            b++;
        const size_t n = b - a;
        std::vector<const uint8_t *> files(n);
        std::vector<uint64_t> sizes(n), offsets(n);
        std::vector<ochip_jpeg_file_info> info(n);
        for (size_t i = 0; i < n; i++)
            files[i] = entries[a + i].data, sizes[i] = entries[a + i].size, offsets[i] = entries[a + i].slot * slot_bytes;
        if (och_jpeg_decoder_decode(dec, (int64_t)n, files.data(), sizes.data(), 1, block, block_bytes, offsets.data(), info.data(),
                                    nullptr) != 0)
        {
            rc = bad(och_jpeg_decode_last_error());
            break;
        }
        for (size_t i = 0; i < n; i++)
        {
            const entry &e = entries[a + i];
            if (info[i].status < 0 || info[i].status > 2)
                rc = bad("a status outside the three");
            else if (info[i].status == OCHIP_JPEG_OK && (info[i].width != e.width || info[i].height != e.height || info[i].offset != offsets[i]))
                rc = bad("file " + std::to_string(a + i) + " went elsewhere or has another size than the list says");
            else
                std::printf("%d %llu %s\n", e.call, (unsigned long long)e.slot, names[info[i].status]);
        }
        a = b;
    }
    och_jpeg_decoder_destroy(dec);
    if (rc == 0)
    {
        std::ofstream out(argv[4], std::ios::binary);
        out.write(reinterpret_cast<const char *>(block), (std::streamsize)block_bytes);
        if (!out)
            rc = bad("cannot write the block");
    }
    std::free(block);
    for (entry &e : entries)
        std::free(e.data);
    return rc;
}
