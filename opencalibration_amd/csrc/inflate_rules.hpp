// INFLATE as this project reads it (RFC 1950 / 1951): the rules for every route that opens a zlib stream - the PNG decoder
// of the host library (host/png_decode.hpp), the GeoTIFF tile reader's host loops (host/geotiff_read.cpp) and its kernels
// (geotiff_read.hip).  The zlib header check, an LSB-first bit reader bounded by the stream's end,
// the code-length code and the two dynamic codes from one length sequence, the fixed codes, the table build with its
// validation, the symbol decode, the length and distance bases, the stored block's LEN / NLEN check, and the host inflate
// that runs them in a loop.  The Adler-32 and its combination are deflate_rules.hpp's.  What is accepted and refused is what
// zlib's inflate decides: an over-subscribed code is refused; an incomplete one too, except a single code of one bit, for
// distances (this project's encoder and zlib both declare it for a block without matches) and for literals/lengths alike
// (zlib's `max != 1` rule; never for the code-length code); a literal/length code without symbol 256; symbols 286 / 287
// and distance symbols 30 / 31 where they are met; a distance beyond the bytes produced.  A stream
// is OK only if it produced exactly the `expect` bytes the caller named, its last block had BFINAL, the Adler-32 matched
// and nothing follows it.  Everything is sized from `expect`, never from what the stream says.  It includes nothing but
// deflate_rules.hpp, so a stand-alone program builds from it.
#pragma once

#include "deflate_rules.hpp"

#define OCHIP_INF_HD OCHIP_DF_HD

namespace ochip_inf
{

constexpr int INF_OK = 0, INF_CORRUPT = 1;
constexpr int FAST_BITS = 9, MAX_BITS = 15; // a first-level lookup of 9 bits, the longer codes by the canonical walk
constexpr int MAX_LIT = 288, MAX_DIST = 32, MAX_LENS = 320;
constexpr uint64_t MAX_RATIO = 1032; // deflate expands at most 1032 : 1 (258 bytes from a two-bit pair of codes)

OCHIP_INF_HD bool zlib_header_ok(uint32_t cmf, uint32_t flg) // CM 8, CINFO <= 7, FCHECK, no FDICT
{
    return (cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8 | flg) % 31) == 0 && !(flg & 0x20);
}

// length symbol 257 .. 285 -> its base (extra bits: ochip_df::length_extra_bits); distance symbol 0 .. 29 likewise
OCHIP_INF_HD constexpr uint32_t length_base(int sym)
{
    return sym < 265 ? (uint32_t)(sym - 254) : sym == 285 ? 258u : 3u + ((4u + (uint32_t)((sym - 261) & 3)) << ((sym - 261) / 4));
}
OCHIP_INF_HD constexpr uint32_t distance_base(int sym)
{
    return sym < 4 ? (uint32_t)(sym + 1) : 1u + ((2u + (uint32_t)(sym & 1)) << (sym / 2 - 1));
}
static_assert(length_base(257) == 3 && length_base(264) == 10 && length_base(265) == 11 && length_base(269) == 19 && length_base(284) == 227 &&
                  length_base(285) == 258,
              "RFC 1951 3.2.5, lengths");
static_assert(distance_base(0) == 1 && distance_base(3) == 4 && distance_base(4) == 5 && distance_base(5) == 7 && distance_base(28) == 16385 &&
                  distance_base(29) == 24577,
              "RFC 1951 3.2.5, distances");

// 4 samples of 8 bits added lane by lane mod 256 in one word (the un-predictor of TIFF's Predictor 2)
OCHIP_INF_HD constexpr uint32_t add_bytes(uint32_t a, uint32_t b)
{
    return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}
static_assert(add_bytes(0xFF01807Fu, 0x01FF8001u) == 0x00000080u, "bytes wrap on their own");

// A stream's bytes as little-endian 32-bit words, zeros behind its end: what a bit reader reads through
struct byte_source
{
    const uint8_t *p;
    uint64_t n;
    OCHIP_INF_HD uint32_t word(uint64_t i) const
    {
        const uint64_t at = 4 * i;
        uint32_t w = 0;
        for (uint64_t k = 0; k < 4; k++)
            if (at + k < n)
                w |= (uint32_t)p[at + k] << (8 * k);
        return w;
    }
};

// Bits LSB first.  Every read is bounded by the stream's end (the source gives zeros behind it); a read past the end
// returns those zeros and sets `ended`, which no caller's loop outlives.
template <class Source> struct bit_reader
{
    Source src;
    uint64_t total_bits; // 8 n
    uint64_t acc = 0;
    uint32_t cnt = 0;  // the bits held in acc
    uint64_t next = 0; // the next word of the source
    bool ended = false;

    OCHIP_INF_HD bit_reader(Source s, uint64_t n) : src(s), total_bits(8 * n) {}
    OCHIP_INF_HD uint64_t bit_pos() const
    {
        return 32 * next - cnt;
    }
    OCHIP_INF_HD uint32_t peek(int k) // k <= 32
    {
        if (cnt <= 32)
            acc |= (uint64_t)src.word(next++) << cnt, cnt += 32;
        return (uint32_t)(acc & (((uint64_t)1 << k) - 1));
    }
    OCHIP_INF_HD void drop(int k) // k <= what peek held
    {
        acc >>= k, cnt -= (uint32_t)k;
        if (bit_pos() > total_bits)
            ended = true;
    }
    OCHIP_INF_HD uint32_t take(int k)
    {
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    OCHIP_INF_HD void align() // to the next byte boundary
    {
        drop((int)(cnt & 7));
    }
    OCHIP_INF_HD void seek_byte(uint64_t at) // a byte position of the stream, at most its end
    {
        next = at / 4, acc = 0, cnt = 0;
        peek(0);
        drop((int)(8 * (at % 4)));
    }
    OCHIP_INF_HD bool at_end() const
    {
        return bit_pos() == total_bits;
    }
};

struct huffman
{
    uint16_t count[MAX_BITS + 1];
    uint16_t symbol[MAX_LIT];
    uint16_t fast[1 << FAST_BITS]; // symbol << 4 | length for the codes of up to FAST_BITS bits, 0: a longer code or none
    uint16_t offs[MAX_BITS + 1], code[MAX_BITS + 1]; // build's work: in the table, so in LDS on the device and not in scratch
};

// A value every lane of the wavefront holds alike, said so that the compiler keeps it in a scalar register; the host: as is
OCHIP_INF_HD uint32_t uniform(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}

// false: over-subscribed, or incomplete in a way inflate refuses (more than a single code of one bit; never for the
// code-length code)
OCHIP_INF_HD bool build(huffman &h, const uint8_t *lens, int n, bool may_be_single)
{
    for (int i = 0; i <= MAX_BITS; i++)
        h.count[i] = 0;
    for (int i = 0; i < n; i++)
        h.count[lens[i] & 15]++;
    int left = 1, longest = 0;
    for (int l = 1; l <= MAX_BITS; l++)
    {
        left <<= 1, left -= h.count[l];
        if (left < 0)
            return false;
        if (h.count[l])
            longest = l;
    }
    if (left > 0 && longest != 0 && !(may_be_single && longest == 1))
        return false;
    if (longest == 0 && !may_be_single)
        return false;
    // offs: where a length's symbols start in canonical order; code: the length's next canonical code
    uint16_t *offs = h.offs, *code = h.code;
    offs[1] = 0, code[1] = 0;
    for (int l = 1; l < MAX_BITS; l++)
    {
        offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
        code[l + 1] = (uint16_t)((code[l] + h.count[l]) << 1);
    }
    for (int i = 0; i < (1 << FAST_BITS); i++)
        h.fast[i] = 0;
    for (int i = 0; i < n; i++)
    {
        const int l = lens[i] & 15;
        if (!l)
            continue;
        h.symbol[offs[l]++] = (uint16_t)i;
        const uint32_t c = code[l]++;
        if (l <= FAST_BITS)
            for (uint32_t k = ochip_df::reverse_bits(c, l); k < (1u << FAST_BITS); k += 1u << l)
                h.fast[k] = (uint16_t)(i << 4 | l);
    }
    return true;
}

// -1: no such code.  A code cut off by the stream's end decodes against the zeros behind it and sets in.ended.
template <class Reader> OCHIP_INF_HD int decode(Reader &in, const huffman &h)
{
    const uint32_t v = in.peek(MAX_BITS);
    const uint32_t e = uniform(h.fast[v & ((1u << FAST_BITS) - 1)]);
    if (e)
    {
        in.drop((int)(e & 15));
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= MAX_BITS; l++)
    {
        code |= (int)((v >> (l - 1)) & 1);
        const int count = (int)uniform(h.count[l]);
        if (code - count < first)
        {
            in.drop(l);
            return (int)uniform(h.symbol[index + (code - first)]);
        }
        index += count, first += count, first <<= 1, code <<= 1;
    }
    return -1;
}

OCHIP_INF_HD void fixed_lengths(uint8_t *lens) // [MAX_LENS]: 288 literal / length codes, then 32 distance codes
{
    for (int i = 0; i < MAX_LIT; i++)
        lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < MAX_DIST; i++) // 30 and 31 complete the code and are refused where they occur
        lens[MAX_LIT + i] = 5;
}

// A dynamic block's code description, behind BTYPE: HLIT, HDIST, HCLEN, the code-length code (built in `cl`) and the one
// sequence of hlit + hdist lengths with its repeats 16 / 17 / 18 into lens[0, hlit + hdist).  false: refused.
template <class Reader> OCHIP_INF_HD bool read_dynamic_lengths(Reader &in, huffman &cl, uint8_t *lens, int &hlit, int &hdist)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    hlit = (int)in.take(5) + 257, hdist = (int)in.take(5) + 1;
    const int hclen = (int)in.take(4) + 4;
    if (in.ended || hlit > 286 || hdist > 30)
        return false;
    for (int i = 0; i < 19; i++)
        lens[i] = 0;
    for (int i = 0; i < hclen; i++)
        lens[order[i]] = (uint8_t)in.take(3);
    if (in.ended || !build(cl, lens, 19, false))
        return false;
    for (int i = 0; i < hlit + hdist;)
    {
        const int s = decode(in, cl);
        if (s < 0 || in.ended)
            return false;
        if (s < 16)
        {
            lens[i++] = (uint8_t)s;
            continue;
        }
        int rep, val = 0;
        if (s == 16)
        {
            if (i == 0)
                return false;
            val = lens[i - 1], rep = 3 + (int)in.take(2);
        }
        else
            rep = s == 17 ? 3 + (int)in.take(3) : 11 + (int)in.take(7);
        if (in.ended || i + rep > hlit + hdist)
            return false;
        while (rep--)
            lens[i++] = (uint8_t)val;
    }
    return lens[256] != 0; // no end-of-block code: refused
}

// A block's two tables from its header, behind BTYPE 1 or 2.  lens: MAX_LENS bytes of work.
template <class Reader> OCHIP_INF_HD bool read_block_codes(Reader &in, uint32_t type, huffman &lit, huffman &dist, uint8_t *lens)
{
    if (type == 1)
    {
        fixed_lengths(lens);
        return build(lit, lens, MAX_LIT, false) && build(dist, lens + MAX_LIT, MAX_DIST, true);
    }
    int hlit = 0, hdist = 0;
    if (!read_dynamic_lengths(in, dist, lens, hlit, hdist)) // the distance table's room holds the code-length code first
        return false;
    return build(lit, lens, hlit, true) && build(dist, lens + hlit, hdist, true);
}

// A stored block behind the byte alignment: LEN and its complement.  false: they disagree or the stream ended.
template <class Reader> OCHIP_INF_HD bool read_stored_length(Reader &in, uint32_t &len)
{
    in.align();
    len = in.take(16);
    const uint32_t nlen = in.take(16);
    return !in.ended && (len ^ 0xFFFFu) == nlen;
}

// What stands behind the last block: the Adler-32, big-endian from the next byte boundary, and then the stream's end
template <class Reader> OCHIP_INF_HD bool read_trailer(Reader &in, uint32_t &adler)
{
    in.align();
    adler = 0;
    for (int i = 0; i < 4; i++)
        adler = adler << 8 | in.take(8);
    return !in.ended && in.at_end(); // bytes behind the Adler-32: trailing garbage inside the stream
}

// Whether a stream of n bytes can be one of `expect` bytes at all, before anything is sized from expect
OCHIP_INF_HD bool plausible(uint64_t n, uint64_t expect)
{
    return n >= 6 && expect <= ((uint64_t)1 << 40) && expect <= n * MAX_RATIO;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host route: the same rules in a loop --------------------------------------------------------------------------------
struct stream_result
{
    int status = INF_CORRUPT;
    uint64_t bytes = 0; // produced, at most expect
};

// The zlib stream z[n] into out[expect]
inline stream_result inflate_stream(const uint8_t *z, uint64_t n, uint8_t *out, uint64_t expect)
{
    stream_result R;
    if (!z || !plausible(n, expect))
        return R;
    bit_reader<byte_source> in(byte_source{z, n}, n);
    const uint32_t cmf = in.take(8), flg = in.take(8);
    if (!zlib_header_ok(cmf, flg))
        return R;
    uint64_t &have = R.bytes;
    huffman lit, dist;
    uint8_t lens[MAX_LENS];
    for (bool last = false; !last;)
    {
        last = in.take(1) != 0;
        const uint32_t type = in.take(2);
        if (in.ended || type == 3)
            return R;
        if (type == 0)
        {
            uint32_t len = 0;
            if (!read_stored_length(in, len) || have + len > expect)
                return R;
            const uint64_t at = in.bit_pos() / 8;
            if (at + len > n)
                return R;
            if (len)
                std::memcpy(out + have, z + at, len);
            have += len;
            in.seek_byte(at + len);
            continue;
        }
        if (!read_block_codes(in, type, lit, dist, lens))
            return R;
        for (;;)
        {
            const int s = decode(in, lit);
            if (s < 0 || in.ended)
                return R;
            if (s < 256)
            {
                if (have >= expect)
                    return R;
                out[have++] = (uint8_t)s;
                continue;
            }
            if (s == 256)
                break;
            if (s > 285)
                return R;
            const uint32_t len = length_base(s) + in.take(ochip_df::length_extra_bits(s));
            const int ds = decode(in, dist);
            if (ds < 0 || ds > 29)
                return R;
            const uint32_t d = distance_base(ds) + in.take(ochip_df::distance_extra_bits(ds));
            if (in.ended || d > have || have + len > expect)
                return R;
            for (uint32_t i = 0; i < len; i++, have++)
                out[have] = out[have - d];
        }
    }
    uint32_t adler = 0;
    if (have != expect || !read_trailer(in, adler))
        return R;
    // combined from the segments' partials, as the device's check pass combines them
    uint32_t a1 = 1, a2 = 0;
    for (uint64_t lo = 0; lo < expect; lo += ochip_df::SEGMENT)
    {
        const uint64_t k = expect - lo < (uint64_t)ochip_df::SEGMENT ? expect - lo : (uint64_t)ochip_df::SEGMENT;
        const uint32_t ad = ochip_df::adler32(out + lo, (size_t)k);
        ochip_df::adler_combine(a1, a2, ad & 0xFFFF, ad >> 16, (uint32_t)k);
    }
    if (adler == (a2 << 16 | a1))
        R.status = INF_OK;
    return R;
}
#endif

// ---- the GeoTIFF tile as it is read -------------------------------------------------------------------
// A tile is tile_w x tile_h pixels of `samples` bytes (PlanarConfiguration 1) or of one float32; its zlib stream inflates to
// exactly tile_bytes; Predictor 2 is undone per tile row - bytes per channel mod 256, a float's 32-bit pattern mod 2^32 - and
// the row is placed into the raster, clipped at its right and bottom edges and cropped to the requested row window.
constexpr int MAX_STREAMS = 65535;                  // a call's most streams
constexpr uint64_t MAX_EXPECT = (uint64_t)1 << 30;  // a stream's most bytes in the inflate of the C ABI
constexpr uint64_t MAX_TILE_BYTES = (uint64_t)4 << 20;
constexpr int64_t MAX_SIDE = 1048576;
constexpr int MAX_READ_LAYERS = 2; // 2 layers of ids in a 512 x 512 tile are the 4 MiB

struct tile_layout
{
    int32_t samples = 0, is_float = 0, tile_w = 0, tile_h = 0, predictor = 1;
    // The layers and cameras rasters: layers > 0, a pixel is `layers` samples of `unit` 32-bit words
    // - B G R A bytes (unit 1, the predictor over bytes) or the two words of a 64-bit id (unit 2, over words) - interleaved
    // in the tile and placed layer-major, [layers][rows][width], in the raster.  samples and is_float are 0 then.
    int32_t layers = 0, unit = 1;
    int64_t width = 0, height = 0;
    OCHIP_INF_HD int64_t pixel_bytes() const
    {
        return layers ? 4 * unit * layers : is_float ? 4 : samples;
    }
    OCHIP_INF_HD bool word_predictor() const // 32-bit sums; else bytes
    {
        return layers ? unit == 2 : is_float != 0;
    }
    OCHIP_INF_HD uint64_t tile_bytes() const
    {
        return (uint64_t)tile_w * (uint64_t)tile_h * (uint64_t)pixel_bytes();
    }
    OCHIP_INF_HD int64_t tiles_x() const
    {
        return (width + tile_w - 1) / tile_w;
    }
    OCHIP_INF_HD int64_t tiles_y() const
    {
        return (height + tile_h - 1) / tile_h;
    }
};

// nullptr, or why the layout is not one this reader takes
inline const char *refuse_layout(const tile_layout &L)
{
    if (L.layers ? (L.layers > MAX_READ_LAYERS || (L.unit != 1 && L.unit != 2)) : L.is_float ? L.samples != 1
                                                                                             : (L.samples != 1 && L.samples != 3 && L.samples != 4))
        return L.layers ? "the layers (kind 2) and cameras (kind 3) rasters have 1 or 2 layers" : "8-bit samples come 1, 3 or 4 to a pixel, float32 one";
    if (L.width < 1 || L.height < 1 || L.width > MAX_SIDE || L.height > MAX_SIDE)
        return "the raster's sides are 1 .. 1048576";
    if (L.tile_w < 16 || L.tile_h < 16 || L.tile_w % 16 != 0 || L.tile_h % 16 != 0 || L.tile_w > 65536 || L.tile_h > 65536)
        return "a tile's sides are multiples of 16";
    if (L.tile_bytes() > MAX_TILE_BYTES)
        return "a tile's payload is at most 4 MiB";
    if (L.predictor != 1 && L.predictor != 2)
        return "the predictor is 1 or 2";
    return nullptr;
}

// The layout of a layers (kind 2) or cameras (kind 3) raster of num_layers layers into L; nullptr, or why it is refused
inline const char *layered_layout(tile_layout &L, int kind, int num_layers, int64_t width, int64_t height, int tile_w, int tile_h, int predictor)
{
    if ((kind != 2 && kind != 3) || num_layers < 1 || num_layers > MAX_READ_LAYERS)
        return "the layers (kind 2) and cameras (kind 3) rasters have 1 or 2 layers";
    L = tile_layout();
    L.layers = num_layers, L.unit = kind == 3 ? 2 : 1, L.tile_w = tile_w, L.tile_h = tile_h, L.predictor = predictor;
    L.width = width, L.height = height;
    return refuse_layout(L);
}

// The tile rows [ty0, ty1) that cover raster rows [row0, row0 + rows); false: the window is not inside the raster
inline bool window_tile_rows(const tile_layout &L, int64_t row0, int64_t rows, int64_t &ty0, int64_t &ty1)
{
    if (row0 < 0 || rows < 0 || row0 > L.height || rows > L.height - row0)
        return false;
    ty0 = row0 / L.tile_h, ty1 = rows == 0 ? ty0 : (row0 + rows + L.tile_h - 1) / L.tile_h;
    return true;
}

// A payload's room in a buffer of payloads: 16-byte vectors store it
OCHIP_INF_HD constexpr uint64_t slot_of(uint64_t expect)
{
    return (expect + 15) & ~(uint64_t)15;
}

// nullptr, or why a call's streams are refused: the same words on both routes
inline const char *refuse_streams(int64_t n, const uint8_t *streams, const uint64_t *offsets)
{
    if (n < 0 || n > MAX_STREAMS)
        return "0 .. 65535 streams a call";
    if (n == 0)
        return nullptr;
    if (!offsets)
        return "the offsets are NULL";
    for (int64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i])
            return "the offsets descend";
    if (!streams && offsets[n] > offsets[0])
        return "the streams are NULL";
    return nullptr;
}

inline const char *refuse_inflate(int64_t n, const uint8_t *streams, const uint64_t *offsets, const uint64_t *expect, const uint8_t *out,
                                  uint64_t out_cap, const int32_t *status, const uint64_t *bytes)
{
    if (const char *why = refuse_streams(n, streams, offsets))
        return why;
    if (n == 0)
        return nullptr;
    if (!expect || !status || !bytes)
        return "expect, status or bytes is NULL";
    uint64_t total = 0; // the last payload needs no more than its bytes
    for (int64_t i = 0; i < n; i++)
    {
        if (expect[i] > MAX_EXPECT)
            return "a stream's expected size is at most 2^30";
        total += i + 1 < n ? slot_of(expect[i]) : expect[i];
    }
    if (total > out_cap || (!out && total > 0))
        return "out is NULL or smaller than the payloads' slots";
    return nullptr;
}

inline const char *refuse_read(const tile_layout &L, int64_t n, const uint8_t *streams, const uint64_t *offsets, int64_t row0, int64_t rows,
                               const void *raster, const int64_t *bad_tile)
{
    int64_t ty0 = 0, ty1 = 0;
    if (!window_tile_rows(L, row0, rows, ty0, ty1))
        return "the row window is not inside the raster";
    if (!bad_tile)
        return "bad_tile is NULL";
    if (n != (ty1 - ty0) * L.tiles_x())
        return "the streams are not those of the tile rows that cover the window";
    if (const char *why = refuse_streams(n, streams, offsets))
        return why;
    if (rows > 0 && !raster)
        return "the raster is NULL";
    return nullptr;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Tile (tx, ty)'s payload - nullptr: a sparse tile, zeros - un-predicted row by row into raster, which holds rows
// [row0, row0 + rows) of the raster.  The payload is changed.
inline void place_tile(const tile_layout &L, uint8_t *payload, int64_t tx, int64_t ty, int64_t row0, int64_t rows, uint8_t *raster)
{
    const int64_t bpp = L.pixel_bytes(), x0 = tx * L.tile_w;
    const int64_t cols = L.width - x0 < L.tile_w ? L.width - x0 : L.tile_w;
    for (int64_t r = 0; r < L.tile_h; r++)
    {
        const int64_t y = ty * L.tile_h + r;
        if (y < row0 || y >= row0 + rows || y >= L.height)
            continue;
        uint8_t *dst = raster + ((size_t)(y - row0) * (size_t)L.width + (size_t)x0) * (size_t)bpp;
        if (!payload)
        {
            if (!L.layers)
                std::memset(dst, 0, (size_t)(cols * bpp));
            for (int64_t l = 0; l < L.layers; l++) // the same pixels of every layer's plane
                std::memset(raster + (((size_t)l * (size_t)rows + (size_t)(y - row0)) * (size_t)L.width + (size_t)x0) * (size_t)(4 * L.unit), 0,
                            (size_t)(cols * 4 * L.unit));
            continue;
        }
        uint8_t *row = payload + (size_t)r * (size_t)L.tile_w * (size_t)bpp;
        if (L.layers)
        {
            // sums at the stride of the pixel, then every layer's sample to its own plane of the raster
            const int64_t W = bpp / 4, sample = 4 * L.unit;
            if (L.predictor == 2 && L.unit == 2)
                for (int64_t k = W; k < cols * W; k++)
                {
                    uint32_t v, left;
                    std::memcpy(&v, row + 4 * k, 4), std::memcpy(&left, row + 4 * (k - W), 4);
                    v += left;
                    std::memcpy(row + 4 * k, &v, 4);
                }
            else if (L.predictor == 2)
                for (int64_t x = bpp; x < cols * bpp; x++)
                    row[x] = (uint8_t)(row[x] + row[x - bpp]);
            for (int64_t l = 0; l < L.layers; l++)
            {
                uint8_t *plane = raster + (((size_t)l * (size_t)rows + (size_t)(y - row0)) * (size_t)L.width + (size_t)x0) * (size_t)sample;
                for (int64_t x = 0; x < cols; x++)
                    std::memcpy(plane + x * sample, row + x * bpp + l * sample, (size_t)sample);
            }
            continue;
        }
        if (L.predictor == 2 && L.is_float)
        {
            uint32_t left = 0;
            for (int64_t x = 0; x < cols; x++)
            {
                uint32_t v;
                std::memcpy(&v, row + 4 * x, 4);
                left += v;
                std::memcpy(row + 4 * x, &left, 4);
            }
        }
        else if (L.predictor == 2)
            for (int64_t x = bpp; x < cols * bpp; x++)
                row[x] = (uint8_t)(row[x] + row[x - bpp]);
        std::memcpy(dst, row, (size_t)(cols * bpp));
    }
}
#endif

} // namespace ochip_inf
