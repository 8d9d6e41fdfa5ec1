// DEFLATE as this project writes it: the zlib stream of a payload of F bytes, one block per 16 384-byte segment, with two match
// candidates - a fixed distance to the left and, optionally, a fixed distance up (a pixel and a row back).  This header is the
// rules for every route and both formats that use them: the match candidates and the greedy parse, the length-limited Huffman
// code with its tie-breaks, the dynamic block header, the choice between the fixed and the dynamic code, the stored fallback,
// the Adler-32 combination, and the host encoder that runs them in loops.  The GeoTIFF tiles (its
// geometry is the last part of this file) and the PNG files (section 4.20, png_rules.hpp) instantiate them; deflate_kernels.hpp
// runs them in kernels.  It includes nothing of either, so a stand-alone program builds from it.  Any valid stream that
// inflates to the payload is correct; the routes give the same bytes because every decision below is a function of the payload
// and the two distances alone.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define OCHIP_DF_HD __host__ __device__ inline
#else
#define OCHIP_DF_HD inline
#endif

namespace ochip_df
{

// One deflate block per segment of the payload, the last with BFINAL
constexpr int SEGMENT = 16384;
constexpr int STORED_BLOCK = 65535; // a stored block's most bytes
// Match candidates: dist_left bytes back and, where there is one, dist_up bytes back.  A position takes the longer run of at
// least MIN_MATCH bytes, the smaller distance on a tie.
constexpr int MIN_MATCH = 4, MAX_MATCH = 258;
constexpr int NO_UP = 0; // as dist_up: no second candidate
// A position's mark: the token's length (0: a literal), the distance chosen, and whether the greedy parse starts a token here
constexpr uint16_t MARK_LEN = 0x1FF, MARK_UP = 0x4000, MARK_START = 0x8000;

constexpr int NUM_LIT = 286, NUM_DIST = 30, NUM_CL = 19, NUM_SYMS = NUM_LIT + NUM_DIST, EOB = 256;
constexpr int HEADER_WORDS = 144; // 17 + 19 x 3 + 316 x 14 = 4 498 bits at most
constexpr uint32_t ADLER_MOD = 65521;

OCHIP_DF_HD constexpr uint64_t segments_of(uint64_t F)
{
    return (F + SEGMENT - 1) / SEGMENT;
}

// The stored form: 78 9C, ceil(F / 65 535) stored blocks of 5 bytes of header each, the Adler-32
OCHIP_DF_HD constexpr uint64_t stored_bytes(uint64_t F)
{
    return 2 + F + 5 * ((F + STORED_BLOCK - 1) / STORED_BLOCK) + 4;
}
static_assert(stored_bytes(1) == 12 && stored_bytes(65535) == 65535 + 11 && stored_bytes(65536) == 65536 + 16, "the stored form");

// A deflated stream of stream_bits is taken only where it is smaller than the stored form, so no stream is larger than that
OCHIP_DF_HD bool takes_deflated(uint64_t stream_bits, uint64_t F, uint64_t &bytes)
{
    bytes = 2 + (stream_bits + 7) / 8 + 4;
    return bytes < stored_bytes(F);
}

OCHIP_DF_HD uint16_t choose_match(int left, int up)
{
    left = left < MAX_MATCH ? left : MAX_MATCH, up = up < MAX_MATCH ? up : MAX_MATCH;
    if (up > left && up >= MIN_MATCH)
        return (uint16_t)(up | MARK_UP);
    return (uint16_t)(left >= MIN_MATCH ? left : 0);
}

OCHIP_DF_HD int floor_log2(uint32_t v) // v > 0
{
    int n = 0;
    while (v >>= 1)
        n++;
    return n;
}

// length 3 .. 258 -> symbol 257 .. 285, its extra bits and their value
OCHIP_DF_HD int length_symbol(int len, int &extra_bits, int &extra)
{
    const int l = len - 3;
    extra_bits = 0, extra = 0;
    if (len == 258)
        return 285;
    if (l < 8)
        return 257 + l;
    extra_bits = floor_log2((uint32_t)l) - 2;
    extra = l & ((1 << extra_bits) - 1);
    return 257 + 4 * (extra_bits + 1) + ((l >> extra_bits) & 3);
}

// distance 1 .. 32 768 -> symbol 0 .. 29
OCHIP_DF_HD int distance_symbol(int dist, int &extra_bits, int &extra)
{
    const int d = dist - 1;
    extra_bits = 0, extra = 0;
    if (d < 4)
        return d;
    extra_bits = floor_log2((uint32_t)d) - 1;
    extra = d & ((1 << extra_bits) - 1);
    return 2 * extra_bits + 2 + ((d >> extra_bits) & 1);
}

OCHIP_DF_HD int length_extra_bits(int sym) // sym 257 .. 285
{
    return sym < 265 || sym == 285 ? 0 : (sym - 261) / 4;
}

OCHIP_DF_HD int distance_extra_bits(int sym)
{
    return sym < 4 ? 0 : sym / 2 - 1;
}

OCHIP_DF_HD uint32_t reverse_bits(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; i++)
        r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// What one block's code construction works in: LDS on the device (a lane's private arrays would be scratch), a local on the
// host.  counts: [0, 286) literals and lengths without the end-of-block symbol, [286, 316) distances.
struct block_work
{
    uint32_t counts[NUM_SYMS];
    uint32_t key[NUM_LIT];
    uint16_t sym[NUM_LIT];
    uint8_t lens[NUM_SYMS];
    uint16_t cl[NUM_SYMS]; // the code-length symbols of the header: symbol | extra value << 8
    uint32_t cl_counts[NUM_CL];
    uint8_t cl_lens[NUM_CL];
    uint32_t cl_codes[NUM_CL];
    uint32_t num[17], next[17];
};

// Code lengths of at most `limit` bits for the n counts: lens[s] = 0 for a count of 0.  The used symbols are sorted by
// (count, symbol) ascending; Moffat and Katajainen's in-place construction gives the Huffman depths in that order (two equal
// weights: the leaf before the internal node, the earlier of either kind first); depths beyond the limit are cut to it and
// the Kraft sum is repaired by lengthening the shortest-lived codes one at a time (the deepest length below the limit that
// has a code gives one up, two appear a level deeper); the lengths then go to the symbols in sorted order, the most frequent
// the shortest.  One used symbol: length 1.  So a more frequent symbol never has a longer code, and with two or more symbols
// the Kraft sum is exactly 1.
OCHIP_DF_HD void code_lengths(const uint32_t *counts, int n, int limit, uint8_t *lens, uint32_t *key, uint16_t *sym, uint32_t *num)
{
    int used = 0;
    for (int s = 0; s < n; s++)
    {
        lens[s] = 0;
        const uint32_t c = counts[s];
        if (c == 0)
            continue;
        int j = used++;
        while (j > 0 && key[j - 1] > c)
            key[j] = key[j - 1], sym[j] = sym[j - 1], j--;
        key[j] = c, sym[j] = (uint16_t)s;
    }
    if (used == 0)
        return;
    if (used == 1)
    {
        lens[sym[0]] = 1;
        return;
    }
    // phase 1: internal node weights and parents
    key[0] += key[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < used - 1; next++)
    {
        if (leaf >= used || key[root] < key[leaf])
            key[next] = key[root], key[root++] = (uint32_t)next;
        else
            key[next] = key[leaf++];
        if (leaf >= used || (root < next && key[root] < key[leaf]))
            key[next] += key[root], key[root++] = (uint32_t)next;
        else
            key[next] += key[leaf++];
    }
    // phase 2: internal depths
    key[used - 2] = 0;
    for (int next = used - 3; next >= 0; next--)
        key[next] = key[key[next]] + 1;
    // phase 3: leaf depths, sorted order: the rarest the deepest
    int avail = 1, inner = 0, depth = 0, nxt = used - 1;
    root = used - 2;
    while (avail > 0)
    {
        while (root >= 0 && (int)key[root] == depth)
            inner++, root--;
        while (avail > inner)
            key[nxt--] = (uint32_t)depth, avail--;
        avail = 2 * inner, depth++, inner = 0;
    }
    // the limit
    for (int i = 0; i <= 16; i++)
        num[i] = 0;
    for (int i = 0; i < used; i++)
        num[(int)key[i] < limit ? key[i] : (uint32_t)limit]++;
    uint32_t total = 0;
    for (int i = limit; i > 0; i--)
        total += num[i] << (limit - i);
    while (total > (1u << limit))
    {
        num[limit]--;
        for (int i = limit - 1; i > 0; i--)
            if (num[i])
            {
                num[i]--, num[i + 1] += 2;
                break;
            }
        total--;
    }
    int j = used;
    for (int i = 1; i <= limit; i++)
        for (uint32_t l = num[i]; l > 0; l--)
            lens[sym[--j]] = (uint8_t)i;
}

// Canonical codes, bit-reversed for the LSB-first stream: length << 16 | code
OCHIP_DF_HD void canonical_codes(const uint8_t *lens, int n, uint32_t *codes, uint32_t *num, uint32_t *next)
{
    for (int i = 0; i <= 16; i++)
        num[i] = 0;
    for (int s = 0; s < n; s++)
        num[lens[s]]++;
    num[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int i = 1; i <= 16; i++)
        code = (code + num[i - 1]) << 1, next[i] = code;
    for (int s = 0; s < n; s++)
    {
        const int l = lens[s];
        codes[s] = l ? (uint32_t)l << 16 | reverse_bits(next[l]++, l) : 0;
    }
}

OCHIP_DF_HD uint32_t fixed_code(int s) // s < 286: literal / length; s >= 286: distance s - 286
{
    if (s >= NUM_LIT)
        return 5u << 16 | reverse_bits((uint32_t)(s - NUM_LIT), 5);
    if (s < 144)
        return 8u << 16 | reverse_bits(0x30u + (uint32_t)s, 8);
    if (s < 256)
        return 9u << 16 | reverse_bits(0x190u + (uint32_t)(s - 144), 9);
    if (s < 280)
        return 7u << 16 | reverse_bits((uint32_t)(s - 256), 7);
    return 8u << 16 | reverse_bits(0xC0u + (uint32_t)(s - 280), 8);
}

// Bits LSB first into zeroed 32-bit words: the header of a block
struct word_bits
{
    uint32_t *words;
    uint32_t cap_bits;
    uint32_t bits;
    OCHIP_DF_HD void put(uint32_t v, int n) // n <= 24
    {
        if (n <= 0 || bits + (uint32_t)n > cap_bits)
            return;
        const uint32_t w = bits >> 5, s = bits & 31;
        words[w] |= v << s;
        if (s + (uint32_t)n > 32)
            words[w + 1] |= v >> (32 - s);
        bits += (uint32_t)n;
    }
};

// One block's codes and header from its counts (W.counts, changed here: the end-of-block symbol is counted, and a block
// without a match counts distance symbol 0 once so that a one-bit distance code is declared, which inflate accepts).
// codes[316]: length << 16 | reversed code of every symbol, of the cheaper of the dynamic and the fixed encoding (the fixed
// one on a tie); header: the block's first bits, BFINAL and BTYPE and for a dynamic block the code description, in zeroed
// words.  Returns the bits of the whole block, header_bits those of the header.
OCHIP_DF_HD uint32_t build_block(block_work &W, bool final, uint32_t *codes, uint32_t *header, uint32_t &header_bits)
{
    const uint8_t order[NUM_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    W.counts[EOB] += 1;
    bool any = false;
    for (int s = 0; s < NUM_DIST; s++)
        any = any || W.counts[NUM_LIT + s] != 0;
    if (!any)
        W.counts[NUM_LIT] = 1;
    code_lengths(W.counts, NUM_LIT, 15, W.lens, W.key, W.sym, W.num);
    code_lengths(W.counts + NUM_LIT, NUM_DIST, 15, W.lens + NUM_LIT, W.key, W.sym, W.num);
    int hlit = NUM_LIT, hdist = NUM_DIST;
    while (hlit > 257 && W.lens[hlit - 1] == 0)
        hlit--;
    while (hdist > 1 && W.lens[NUM_LIT + hdist - 1] == 0)
        hdist--;
    // the lengths of both codes as one sequence, runs coded with 16 (repeat 3 - 6), 17 (zeros 3 - 10), 18 (zeros 11 - 138)
    for (int i = 0; i < NUM_CL; i++)
        W.cl_counts[i] = 0;
    const int total = hlit + hdist;
    int ncl = 0;
    for (int i = 0; i < total;)
    {
        const int v = W.lens[i < hlit ? i : NUM_LIT + (i - hlit)];
        int run = 1;
        while (i + run < total && W.lens[i + run < hlit ? i + run : NUM_LIT + (i + run - hlit)] == v)
            run++;
        i += run;
        if (v == 0)
        {
            while (run >= 11)
            {
                const int r = run < 138 ? run : 138;
                W.cl[ncl++] = (uint16_t)(18 | (r - 11) << 8), W.cl_counts[18]++, run -= r;
            }
            if (run >= 3)
                W.cl[ncl++] = (uint16_t)(17 | (run - 3) << 8), W.cl_counts[17]++, run = 0;
        }
        else
        {
            W.cl[ncl++] = (uint16_t)v, W.cl_counts[v]++, run--;
            while (run >= 3)
            {
                const int r = run < 6 ? run : 6;
                W.cl[ncl++] = (uint16_t)(16 | (r - 3) << 8), W.cl_counts[16]++, run -= r;
            }
        }
        for (; run > 0; run--)
            W.cl[ncl++] = (uint16_t)v, W.cl_counts[v]++;
    }
    code_lengths(W.cl_counts, NUM_CL, 7, W.cl_lens, W.key, W.sym, W.num);
    {
        // the code-length code has to be complete: a lone symbol gets a neighbour of length 1 that is never sent
        int used = 0, only = 0;
        for (int i = 0; i < NUM_CL; i++)
            if (W.cl_lens[i])
                used++, only = i;
        if (used == 1)
            W.cl_lens[only == 0 ? 1 : 0] = 1;
    }
    canonical_codes(W.cl_lens, NUM_CL, W.cl_codes, W.num, W.next);
    int hclen = NUM_CL;
    while (hclen > 4 && W.cl_lens[order[hclen - 1]] == 0)
        hclen--;
    uint32_t dynamic = 3 + 14 + 3 * (uint32_t)hclen, fixed = 3;
    for (int k = 0; k < ncl; k++)
    {
        const int s = W.cl[k] & 255;
        dynamic += W.cl_lens[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    for (int s = 0; s < NUM_SYMS; s++)
    {
        const uint32_t c = W.counts[s];
        if (c == 0)
            continue;
        const uint32_t extra = s >= NUM_LIT ? (uint32_t)distance_extra_bits(s - NUM_LIT) : s > EOB ? (uint32_t)length_extra_bits(s) : 0;
        dynamic += c * (W.lens[s] + extra);
        fixed += c * ((fixed_code(s) >> 16) + extra);
    }
    if (!any) // the distance symbol counted above is declared, never sent
        dynamic -= W.lens[NUM_LIT], fixed -= 5;
    word_bits h{header, HEADER_WORDS * 32, 0};
    h.put(final ? 1 : 0, 1);
    if (dynamic < fixed)
    {
        canonical_codes(W.lens, NUM_LIT, codes, W.num, W.next);
        canonical_codes(W.lens + NUM_LIT, NUM_DIST, codes + NUM_LIT, W.num, W.next);
        h.put(2, 2);
        h.put((uint32_t)(hlit - 257), 5), h.put((uint32_t)(hdist - 1), 5), h.put((uint32_t)(hclen - 4), 4);
        for (int i = 0; i < hclen; i++)
            h.put(W.cl_lens[order[i]], 3);
        for (int k = 0; k < ncl; k++)
        {
            const int s = W.cl[k] & 255;
            h.put(W.cl_codes[s] & 0xFFFF, (int)(W.cl_codes[s] >> 16));
            if (s >= 16)
                h.put((uint32_t)(W.cl[k] >> 8), s == 16 ? 2 : s == 17 ? 3 : 7);
        }
    }
    else
    {
        for (int s = 0; s < NUM_SYMS; s++)
            codes[s] = fixed_code(s);
        h.put(1, 2);
    }
    header_bits = h.bits;
    return dynamic < fixed ? dynamic : fixed;
}

// The bits of the token a mark starts: a literal `byte`, or a length and distance pair.  At most 48 bits, LSB first.
OCHIP_DF_HD uint64_t token_bits(uint16_t mark, uint8_t byte, const uint32_t *codes, int &n, int dist_left, int dist_up)
{
    const int len = mark & MARK_LEN;
    if (len == 0)
    {
        const uint32_t c = codes[byte];
        n = (int)(c >> 16);
        return c & 0xFFFF;
    }
    int eb, ev, db, dv;
    const uint32_t lc = codes[length_symbol(len, eb, ev)];
    const uint32_t dc = codes[NUM_LIT + distance_symbol((mark & MARK_UP) ? dist_up : dist_left, db, dv)];
    uint64_t v = lc & 0xFFFF;
    n = (int)(lc >> 16);
    v |= (uint64_t)ev << n, n += eb;
    v |= (uint64_t)(dc & 0xFFFF) << n, n += (int)(dc >> 16);
    v |= (uint64_t)dv << n, n += db;
    return v;
}

// The symbols a mark's token counts: the literal / length symbol, and the distance symbol or -1
OCHIP_DF_HD int token_symbols(uint16_t mark, uint8_t byte, int &dist_sym, int dist_left, int dist_up)
{
    const int len = mark & MARK_LEN;
    dist_sym = -1;
    if (len == 0)
        return byte;
    int eb, ev;
    dist_sym = distance_symbol((mark & MARK_UP) ? dist_up : dist_left, eb, ev);
    return length_symbol(len, eb, ev);
}

// Adler-32 as (s1, s2) of a piece on its own, and of piece a followed by piece b of len_b bytes
OCHIP_DF_HD void adler_combine(uint32_t &s1, uint32_t &s2, uint32_t s1b, uint32_t s2b, uint32_t len_b)
{
    const uint32_t m = ADLER_MOD;
    const uint32_t a1 = (s1 + m - 1) % m; // s1a - 1
    s2 = (uint32_t)((s2 + s2b + (uint64_t)(len_b % m) * a1) % m);
    s1 = (a1 + s1b) % m;
}

// Byte o of the stored form of a payload of F bytes whose Adler-32 is `adler`; o < stored_bytes(F)
OCHIP_DF_HD uint8_t stored_byte(uint64_t o, const uint8_t *payload, uint64_t F, uint32_t adler)
{
    const uint64_t S = stored_bytes(F), blocks = (F + STORED_BLOCK - 1) / STORED_BLOCK;
    if (o < 2)
        return o == 0 ? 0x78 : 0x9C;
    if (o >= S - 4)
        return (uint8_t)(adler >> (8 * (S - 1 - o)));
    const uint64_t k = (o - 2) / (STORED_BLOCK + 5), r = (o - 2) % (STORED_BLOCK + 5);
    if (r >= 5)
        return payload[k * STORED_BLOCK + (r - 5)];
    const uint32_t len = k + 1 < blocks ? (uint32_t)STORED_BLOCK : (uint32_t)(F - k * STORED_BLOCK);
    return r == 0 ? (k + 1 == blocks ? 1 : 0) : r == 1 ? (uint8_t)len : r == 2 ? (uint8_t)(len >> 8) : r == 3 ? (uint8_t)~len : (uint8_t)(~len >> 8);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host route's encoder: the same rules in loops ------------------------------------------------------------------------
inline uint32_t adler32(const uint8_t *p, size_t n)
{
    uint32_t s1 = 1, s2 = 0;
    while (n)
    {
        const size_t k = n < 5552 ? n : 5552;
        for (size_t i = 0; i < k; i++)
            s1 += p[i], s2 += s1;
        s1 %= ADLER_MOD, s2 %= ADLER_MOD, p += k, n -= k;
    }
    return s2 << 16 | s1;
}

struct block_out
{
    uint32_t codes[NUM_SYMS];
    uint32_t header[HEADER_WORDS];
    uint32_t header_bits = 0, bits = 0;
};

// One segment of a payload of F bytes: the candidate runs backwards from its end into marks[lo, hi), the greedy parse from
// its start, the block's codes.  dist_up: NO_UP or the second candidate's distance.
inline void segment_block(const uint8_t *a, uint64_t F, uint64_t seg, int dist_left, int dist_up, uint16_t *marks, block_out &B)
{
    const int64_t lo = (int64_t)seg * SEGMENT, hi = lo + SEGMENT < (int64_t)F ? lo + SEGMENT : (int64_t)F;
    int left = 0, up = 0;
    for (int64_t p = hi - 1; p >= lo; p--)
    {
        left = p >= dist_left && a[p] == a[p - dist_left] ? left + 1 : 0;
        up = dist_up != NO_UP && p >= dist_up && a[p] == a[p - dist_up] ? up + 1 : 0;
        marks[p] = choose_match(left, up);
    }
    block_work W;
    std::memset(W.counts, 0, sizeof W.counts);
    for (int64_t p = lo; p < hi;)
    {
        marks[p] |= MARK_START;
        int ds;
        W.counts[token_symbols(marks[p], a[p], ds, dist_left, dist_up)]++;
        if (ds >= 0)
            W.counts[NUM_LIT + ds]++;
        const int len = marks[p] & MARK_LEN;
        p += len ? len : 1;
    }
    std::memset(B.header, 0, sizeof B.header);
    B.bits = build_block(W, seg + 1 == segments_of(F), B.codes, B.header, B.header_bits);
}

// Bits LSB first into zeroed bytes, the position 64-bit
struct bit_sink
{
    uint8_t *bytes;
    uint64_t cap_bits, bits;
    void put(uint64_t v, int n) // n <= 48
    {
        if (n <= 0 || bits + (uint64_t)n > cap_bits)
            return;
        uint64_t at = bits >> 3;
        const int s = (int)(bits & 7);
        bits += (uint64_t)n;
        unsigned __int128 w = (unsigned __int128)v << s;
        for (int left = n + s; left > 0; left -= 8, w >>= 8)
            bytes[at++] |= (uint8_t)w;
    }
};

// A marked and coded segment's block: the header in 16-bit slices, the tokens, the end-of-block symbol
inline void emit_segment(bit_sink &w, const uint8_t *a, uint64_t F, uint64_t seg, int dist_left, int dist_up, const uint16_t *marks,
                         const block_out &B)
{
    const int64_t lo = (int64_t)seg * SEGMENT, hi = lo + SEGMENT < (int64_t)F ? lo + SEGMENT : (int64_t)F;
    for (uint32_t b = 0; b < B.header_bits; b += 16)
    {
        const int n = B.header_bits - b < 16 ? (int)(B.header_bits - b) : 16;
        w.put((B.header[b >> 5] >> (b & 31)) & ((1u << n) - 1), n);
    }
    for (int64_t p = lo; p < hi; p++)
        if (marks[p] & MARK_START)
        {
            int n;
            const uint64_t v = token_bits(marks[p], a[p], B.codes, n, dist_left, dist_up);
            w.put(v, n);
        }
    w.put(B.codes[EOB] & 0xFFFF, (int)(B.codes[EOB] >> 16));
}

// The bytes of the stream of a payload whose segments are coded, and whether it is the deflated one
inline uint64_t stream_bytes(const block_out *blocks, uint64_t F, bool &deflated)
{
    uint64_t bits = 0, bytes = 0;
    for (uint64_t k = 0; k < segments_of(F); k++)
        bits += blocks[k].bits;
    deflated = takes_deflated(bits, F, bytes);
    return deflated ? bytes : stored_bytes(F);
}

// The stream into z[stream_bytes], zeroed: deflated from the marks and blocks, or stored.  The Adler-32 is combined from the
// segments' partials, as the device combines them.
inline void write_stream(const uint8_t *a, uint64_t F, int dist_left, int dist_up, const uint16_t *marks, const block_out *blocks,
                         bool deflated, uint64_t zlen, uint8_t *z)
{
    uint32_t a1 = 1, a2 = 0;
    for (uint64_t lo = 0; lo < F; lo += SEGMENT)
    {
        const uint64_t n = F - lo < (uint64_t)SEGMENT ? F - lo : (uint64_t)SEGMENT;
        const uint32_t ad = adler32(a + lo, (size_t)n);
        adler_combine(a1, a2, ad & 0xFFFF, ad >> 16, (uint32_t)n);
    }
    const uint32_t adler = a2 << 16 | a1;
    if (!deflated)
    {
        for (uint64_t o = 0; o < zlen; o++)
            z[o] = stored_byte(o, a, F, adler);
        return;
    }
    z[0] = 0x78, z[1] = 0x9C;
    bit_sink w{z, (zlen - 4) * 8, 16};
    for (uint64_t k = 0; k < segments_of(F); k++)
        emit_segment(w, a, F, k, dist_left, dist_up, marks, blocks[k]);
    for (int k = 0; k < 4; k++)
        z[zlen - 4 + k] = (uint8_t)(adler >> (8 * (3 - k)));
}

// The zlib stream of a payload of F bytes into out (cleared first), serially; at most stored_bytes(F)
inline void encode_stream(const uint8_t *a, uint64_t F, int dist_left, int dist_up, std::vector<uint8_t> &out)
{
    std::vector<uint16_t> marks((size_t)F);
    std::vector<block_out> blocks((size_t)segments_of(F));
    for (uint64_t k = 0; k < segments_of(F); k++)
        segment_block(a, F, k, dist_left, dist_up, marks.data(), blocks[(size_t)k]);
    bool deflated = false;
    const uint64_t zlen = stream_bytes(blocks.data(), F, deflated);
    out.assign((size_t)zlen, 0);
    write_stream(a, F, dist_left, dist_up, marks.data(), blocks.data(), deflated, zlen, out.data());
}
#endif

// ---- the GeoTIFF tile (the reference's GDAL options COMPRESS=DEFLATE, PREDICTOR=2 on 512 x 512 tiles,
// src/ortho/ortho.cpp:655-708 and :745-791) -----------------------------------------------------------------------------------
// A tile is 512 x 512 pixels of 4 bytes - RGBA8 or one float32 - so its predicted payload is 1 MiB: 64 segments of 8 tile
// rows, the candidates the pixel to the left and the pixel above.
constexpr int TILE = 512, PIXEL_BYTES = 4, ROW_BYTES = TILE * PIXEL_BYTES;
constexpr int PAYLOAD = TILE * ROW_BYTES; // 1 048 576
constexpr int SEGMENTS = PAYLOAD / SEGMENT;
constexpr int DIST_LEFT = PIXEL_BYTES, DIST_UP = ROW_BYTES;
constexpr int STORED_BLOCKS = (PAYLOAD + STORED_BLOCK - 1) / STORED_BLOCK;
constexpr int STORED_BYTES = (int)stored_bytes(PAYLOAD);
static_assert(STORED_BLOCKS == 17 && STORED_BYTES == 1048667, "the bound every buffer is sized from");
constexpr int TILE_SLOT = (STORED_BYTES + 15) / 16 * 16; // a tile's room in a device buffer

// The layers and cameras rasters between the layer pass and the blend (the reference's
// createMultiBandGeoTIFF, src/ortho/ortho.cpp:969-1008): the same tiles with a wider pixel.  A layers pixel is B G R A of each
// of its L layers, 4 L bytes; a cameras pixel the low and the high 32-bit word of each layer's 64-bit node id, 8 L bytes.  The
// raster comes layer-major, [L][rows][width] units of 1 (B G R A) or 2 (an id) 32-bit words; the payload is pixel-interleaved,
// [row][col][layer][word].  The candidates stay the pixel to the left and the pixel above, so everything above follows from
// the pixel's bytes alone.
constexpr int KIND_RGBA8 = 0, KIND_FLOAT32 = 1, KIND_LAYERS8 = 2, KIND_CAMERAS32 = 3;
constexpr int MAX_LAYERS = 2; // the reference's pipeline never leaves 2; a pixel of 4, 8 or 16 bytes

OCHIP_DF_HD constexpr bool layered_kind(int kind)
{
    return kind == KIND_LAYERS8 || kind == KIND_CAMERAS32;
}
OCHIP_DF_HD constexpr int unit_words(int kind) // the 32-bit words of one layer's sample of a pixel
{
    return kind == KIND_CAMERAS32 ? 2 : 1;
}
OCHIP_DF_HD constexpr int pixel_bytes(int kind, int layers) // layers: 1 for the two kinds without layers
{
    return 4 * unit_words(kind) * layers;
}
OCHIP_DF_HD constexpr bool word_predictor(int kind) // 32-bit differences; else bytes
{
    return kind == KIND_FLOAT32 || kind == KIND_CAMERAS32;
}
OCHIP_DF_HD constexpr int tile_row_bytes(int px)
{
    return TILE * px;
}
OCHIP_DF_HD constexpr int tile_payload(int px)
{
    return TILE * TILE * px;
}
OCHIP_DF_HD constexpr int tile_segments(int px)
{
    return tile_payload(px) / SEGMENT;
}
OCHIP_DF_HD constexpr int tile_stored_bytes(int px)
{
    return (int)stored_bytes((uint64_t)tile_payload(px));
}
OCHIP_DF_HD constexpr int tile_slot(int px) // a tile's room in a device buffer
{
    return (tile_stored_bytes(px) + 15) / 16 * 16;
}
static_assert(tile_payload(PIXEL_BYTES) == PAYLOAD && tile_segments(PIXEL_BYTES) == SEGMENTS && tile_stored_bytes(PIXEL_BYTES) == STORED_BYTES &&
                  tile_slot(PIXEL_BYTES) == TILE_SLOT && tile_row_bytes(PIXEL_BYTES) == DIST_UP,
              "the 4-byte pixel is one case of the geometry");
static_assert(tile_payload(16) == 4 << 20 && tile_row_bytes(16) == 8192 && tile_stored_bytes(16) == 4194304 + 5 * 65 + 6, "two layers of ids");

// The predictor over one tile row of 512 pixels: the first pixel stays, RGBA bytes take the byte 4 before them away, a
// float's 32-bit pattern the pattern before it.  src: the row's pixels as 32-bit words, `valid` of them real, zeros behind.
OCHIP_DF_HD uint32_t predict_word(uint32_t cur, uint32_t left, bool is_float)
{
    if (is_float)
        return cur - left;
    return ((cur | 0x80808080u) - (left & 0x7F7F7F7Fu)) ^ ((cur ^ ~left) & 0x80808080u);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The zlib stream of a tile's payload into out (cleared first); at most STORED_BYTES
inline void encode_tile(const uint8_t *a, std::vector<uint8_t> &out)
{
    encode_stream(a, PAYLOAD, DIST_LEFT, DIST_UP, out);
}

// The same for a tile whose pixel has px bytes; at most tile_stored_bytes(px)
inline void encode_tile(const uint8_t *a, int px, std::vector<uint8_t> &out)
{
    encode_stream(a, (uint64_t)tile_payload(px), px, tile_row_bytes(px), out);
}
#endif

} // namespace ochip_df
