// The DEFLATE encoder on the device (the rules: deflate_rules.hpp): the bodies of the kernels of geotiff.hip and png.hip, which
// both write one block per 16 384-byte segment of a payload, a workgroup of 256 lanes a segment, 64 bytes a lane.  A format's
// kernel finds its tile or image and its segment, applies its own skip rule, makes the lane's two match masks its own way -
// that is where the formats differ; in the kernel's body, because as a function of their own the same statements compile to
// more than twice the registers (profiles/deflate_shared_resource_usage.md) - and calls
//   parse_segment   the runs out of the masks and the heads of the chunks behind (LDS); the greedy parse - a walk from the
//                   segment's start - cut into the lanes' chunks: where a walk that enters a chunk at each of its positions
//                   leaves it (64 steps a lane, all lanes at once), one lane's hops from chunk to chunk (at most 256), then
//                   every entered chunk marks and counts its tokens; the segment's Adler-32 partial
//   codes_block     a wave per block: the counts, the code construction's arrays and the header in LDS, the construction
//                   itself - sequential by nature - on one lane; the block's bits
//   emit_segment    a lane sums the bits of the tokens that start in its 64 bytes, a scan over the workgroup places them,
//                   whole words are stored and the two ragged ones ORed into the zeroed buffer
//   stream_adler, stored_word   a stream's Adler-32 from its segments' partials; a word of the stored form
// and the host side uses scan_offsets for the two exclusive scans (rocPRIM) between them.  Everything is inlined into its
// caller, so a format with fixed geometry (the GeoTIFF tile: distances 4 and 2 048, whole segments) keeps its constants.
#pragma once

#include "ctx.hpp"
#include "deflate_rules.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace ochip_dfk
{

using namespace ochip_df;

constexpr int THREADS = 256, CHUNK = SEGMENT / THREADS; // a lane's 64 bytes of a segment
static_assert(CHUNK == 64, "a lane's bytes are the bits of one 64-bit mask");

__device__ __forceinline__ int ones_from(uint64_t m, int j) // the run of set bits of m from bit j upwards, at most 64 - j
{
    const uint64_t x = ~(m >> j);
    return x ? __builtin_ctzll(x) : 64;
}

// the bits of a mask whose byte of `x` is zero, at bit positions j0 .. j0 + 3
__device__ __forceinline__ uint64_t zero_bytes(uint32_t x, int j0)
{
    uint64_t m = 0;
#pragma unroll
    for (int y = 0; y < 4; y++)
        if (((x >> (8 * y)) & 255u) == 0)
            m |= 1ull << (j0 + y);
    return m;
}

// One segment, bytes [lo, lo + extent) of the payload `a`, extent <= SEGMENT; called by all 256 lanes of the workgroup.  The
// lane's chunk starts at lo + 64 t and has `valid` real bytes (0 .. 64: less than 64 only in a payload's last segment).
// m_left, m_up: bit j is set where byte j of the chunk equals the byte dist_left / dist_up before it (clear beyond valid and
// where there is no such byte); s1, s2: the chunk's byte sum and the sum of (valid - j) byte j.  Writes the marks into
// tok[lo, lo + extent), the block's 316 counts and the segment's Adler-32 partial (s1, s2) into adler2[0 .. 1].
__device__ __forceinline__ void parse_segment(uint64_t m_left, uint64_t m_up, uint32_t s1, uint32_t s2, int valid, const uint8_t *a, uint32_t lo,
                                              uint32_t extent, int dist_left, int dist_up, uint16_t *tok, uint32_t *counts, uint32_t *adler2)
{
    constexpr uint16_t MARK_OVER = 0x200; // a mark's spare bit, inside the parse only
    constexpr int NOT_ENTERED = CHUNK;    // the walk jumps over the chunk
    __shared__ uint16_t best[SEGMENT];
    __shared__ uint8_t leave[SEGMENT];
    __shared__ uint8_t entry[THREADS];
    __shared__ uint16_t head[2][THREADS];
    __shared__ uint32_t cnt[NUM_SYMS];
    __shared__ uint32_t ad1[THREADS], ad2[THREADS];
    const int t = threadIdx.x;
    // a lane without a real byte still publishes an empty chunk: no run, the Adler-32 of nothing
    head[0][t] = (uint16_t)ones_from(m_left, 0), head[1][t] = (uint16_t)ones_from(m_up, 0);
    ad1[t] = 1 + s1, ad2[t] = ((uint32_t)valid + s2) % ADLER_MOD;
    for (int i = t; i < NUM_SYMS; i += THREADS)
        cnt[i] = 0;
    __syncthreads();
    // how far a run that reaches this chunk's end goes on in the chunks behind, the segment's end the limit
    int more[2] = {0, 0};
#pragma unroll
    for (int d = 0; d < 2; d++)
    {
        int r = 0;
        for (int k = t + 1; k < THREADS; k++)
        {
            const int h = head[d][k];
            r += h;
            if (h < CHUNK || r >= MAX_MATCH)
                break;
        }
        more[d] = r;
    }
    for (int j = 0; j < CHUNK; j++)
    {
        int rl = ones_from(m_left, j), ru = ones_from(m_up, j);
        if (rl == CHUNK - j)
            rl += more[0];
        if (ru == CHUNK - j)
            ru += more[1];
        best[t * CHUNK + j] = choose_match(rl, ru);
    }
    // The greedy parse is a walk from the segment's start.  Each lane first finds, for every position of its chunk, how far
    // behind the chunk's end a walk entering there leaves it (0 .. 257: nine bits, the ninth in the mark's spare bit);
    // backwards, so a position reads the answer of the one it steps to.  One lane then hops from chunk to chunk - at most
    // 256 hops instead of 16 384 steps, the chunks beyond the extent included - and every entered chunk marks its own tokens.
    for (int e = CHUNK - 1; e >= 0; e--)
    {
        const uint16_t m = best[t * CHUNK + e];
        const int len = m & MARK_LEN, n = e + (len ? len : 1);
        int over;
        if (n >= CHUNK)
            over = n - CHUNK;
        else
            over = leave[t * CHUNK + n] | ((best[t * CHUNK + n] & MARK_OVER) ? 256 : 0);
        leave[t * CHUNK + e] = (uint8_t)over;
        if (over & 256)
            best[t * CHUNK + e] = m | MARK_OVER;
    }
    entry[t] = NOT_ENTERED;
    __syncthreads();
    if (t == 0)
    {
        for (int c = 0, e = 0; c < THREADS;)
        {
            entry[c] = (uint8_t)e;
            const int at = c * CHUNK + e;
            const int next = (c + 1) * CHUNK + (leave[at] | ((best[at] & MARK_OVER) ? 256 : 0));
            c = next / CHUNK, e = next % CHUNK;
        }
    }
    else if (t == 64)
    {
        uint32_t a1 = ad1[0], a2 = ad2[0];
        for (int k = 1; k < THREADS; k++)
        {
            const uint32_t at = (uint32_t)k * CHUNK;
            adler_combine(a1, a2, ad1[k], ad2[k], at >= extent ? 0 : extent - at < (uint32_t)CHUNK ? extent - at : (uint32_t)CHUNK);
        }
        adler2[0] = a1, adler2[1] = a2;
    }
    __syncthreads();
    // the tokens of this lane's chunk, if the walk enters it: marked and counted in one pass.  No match reaches beyond the
    // segment's end, so the walk steps over the bytes behind it one by one and nothing there is marked.
    const uint8_t *mine = a + lo + (uint32_t)t * CHUNK;
    for (int j = entry[t]; j < valid;)
    {
        const uint16_t m = best[t * CHUNK + j];
        best[t * CHUNK + j] = m | MARK_START;
        int ds;
        const int ls = token_symbols(m, mine[j], ds, dist_left, dist_up);
        atomicAdd(&cnt[ls], 1u);
        if (ds >= 0)
            atomicAdd(&cnt[NUM_LIT + ds], 1u);
        const int len = m & MARK_LEN;
        j += len ? len : 1;
    }
    __syncthreads();
    uint16_t *out = tok + lo;
    for (uint32_t i = t; i < extent; i += THREADS)
        out[i] = best[i] & (uint16_t)~MARK_OVER;
    for (int i = t; i < NUM_SYMS; i += THREADS)
        counts[i] = cnt[i];
}

// One block's codes, header and bits from its 316 counts; called by the 64 lanes of the workgroup.  final: the stream's last
__device__ __forceinline__ void codes_block(const uint32_t *counts, bool final, uint32_t *codes, uint32_t *header, uint32_t *header_bits,
                                            uint32_t *block_bits)
{
    __shared__ block_work W;
    __shared__ uint32_t c[NUM_SYMS];
    __shared__ uint32_t h[HEADER_WORDS];
    __shared__ uint32_t hb;
    const int t = threadIdx.x;
    for (int i = t; i < NUM_SYMS; i += 64)
        W.counts[i] = counts[i];
    for (int i = t; i < HEADER_WORDS; i += 64)
        h[i] = 0;
    __syncthreads();
    if (t == 0)
    {
        uint32_t bits_of_header = 0;
        *block_bits = build_block(W, final, c, h, bits_of_header);
        hb = bits_of_header;
    }
    __syncthreads();
    for (int i = t; i < NUM_SYMS; i += 64)
        codes[i] = c[i];
    for (int i = t; i < HEADER_WORDS; i += 64)
        header[i] = h[i];
    if (t == 0)
        *header_bits = hb;
}

// Bits LSB first from bit `pos` of a stream's words.  A word this lane fills alone is stored; the first word when the lane
// starts inside it and the last partial one are ORed into the zeroed buffer.  Nothing is written at or beyond cap.
struct bit_writer
{
    uint32_t *words;
    uint32_t cap, wi;
    uint64_t acc;
    int n;
    bool shared_first;
    __device__ __forceinline__ bit_writer(uint32_t *words_, uint32_t cap_, unsigned long long pos)
        : words(words_), cap(cap_), wi((uint32_t)(pos >> 5)), acc(0), n((int)(pos & 31)), shared_first((pos & 31) != 0)
    {
    }
    __device__ __forceinline__ void put(uint32_t v, int len) // len <= 24
    {
        acc |= (uint64_t)v << n, n += len;
        if (n >= 32)
        {
            if (wi < cap)
            {
                if (shared_first)
                    atomicOr(&words[wi], (uint32_t)acc);
                else
                    words[wi] = (uint32_t)acc;
            }
            shared_first = false;
            wi++, n -= 32, acc >>= 32;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (n > 0 && wi < cap)
            atomicOr(&words[wi], (uint32_t)acc);
    }
};

// One block into its stream; called by all 256 lanes.  a, marks: the segment's first byte and mark, of which the lane's
// chunk has `valid`; words, cap: the stream's zeroed words and how many may be written; pos: the bit of the stream at which
// the block starts.
__device__ __forceinline__ void emit_segment(const uint8_t *a, const uint16_t *marks, int valid, const uint32_t *codes, const uint32_t *header,
                                             uint32_t hbits, uint32_t *words, uint32_t cap, unsigned long long pos, int dist_left, int dist_up)
{
    __shared__ uint32_t c[NUM_SYMS];
    __shared__ uint32_t sc[THREADS];
    const int t = threadIdx.x;
    for (int i = t; i < NUM_SYMS; i += THREADS)
        c[i] = codes[i];
    __syncthreads();
    a += (size_t)t * CHUNK, marks += (size_t)t * CHUNK;
    uint32_t bits = 0;
    for (int j = 0; j < valid; j++)
    {
        const uint16_t m = marks[j];
        if (m & MARK_START)
        {
            int n;
            (void)token_bits(m, a[j], c, n, dist_left, dist_up);
            bits += (uint32_t)n;
        }
    }
    if (t == 0)
        bits += hbits;
    if (t == THREADS - 1)
        bits += c[EOB] >> 16;
    sc[t] = bits;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1)
    {
        const uint32_t v = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    bit_writer w(words, cap, pos + (sc[t] - bits));
    if (t == 0)
    {
        for (uint32_t at = 0; at < hbits && at < HEADER_WORDS * 32; at += 16) // the header in 16-bit slices
        {
            const int n = hbits - at < 16 ? (int)(hbits - at) : 16;
            w.put((header[at >> 5] >> (at & 31)) & ((1u << n) - 1), n);
        }
    }
    for (int j = 0; j < valid; j++)
    {
        const uint16_t m = marks[j];
        if (m & MARK_START)
        {
            int n;
            const uint64_t v = token_bits(m, a[j], c, n, dist_left, dist_up);
            w.put((uint32_t)(v & 0xFFFFFF), n < 24 ? n : 24);
            if (n > 24)
                w.put((uint32_t)(v >> 24), n - 24);
        }
    }
    if (t == THREADS - 1)
        w.put(c[EOB] & 0xFFFF, (int)(c[EOB] >> 16));
    w.flush();
}

// The Adler-32 of a payload of F bytes from its segments' partials, adler2[2 k], adler2[2 k + 1] of segment k
__device__ __forceinline__ uint32_t stream_adler(const uint32_t *adler2, uint32_t F)
{
    uint32_t a1 = 1, a2 = 0;
    for (uint32_t k = 0, at = 0; at < F; k++, at += SEGMENT)
        adler_combine(a1, a2, adler2[2 * (size_t)k], adler2[2 * (size_t)k + 1], F - at < (uint32_t)SEGMENT ? F - at : (uint32_t)SEGMENT);
    return a2 << 16 | a1;
}

// Word wd of the stored form of a payload of F bytes, zeros behind its end
__device__ __forceinline__ uint32_t stored_word(uint32_t wd, const uint8_t *payload, uint32_t F, uint32_t adler)
{
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
    {
        const uint64_t o = (uint64_t)wd * 4 + k;
        if (o < stored_bytes(F))
            word |= (uint32_t)stored_byte(o, payload, F, adler) << (8 * k);
    }
    return word;
}

// ---- the host side of the launches --------------------------------------------------------------------------------------------
struct widen
{
    __host__ __device__ unsigned long long operator()(uint32_t v) const
    {
        return v;
    }
};

inline uint32_t blocks_of(size_t n)
{
    return (uint32_t)((n + THREADS - 1) / THREADS);
}

inline int launched(ochip_ctx *ctx, const char *what)
{
    return hipGetLastError() == hipSuccess ? OCHIP_OK : ochip_fail(ctx, OCHIP_EHIP, "%s launch failed", what);
}

// The exclusive scan of n 32-bit sizes into 64-bit offsets - the last of the sizes 0, so that the last offset is the total -
// on the stream, with `tmp_bytes` at tmp; a null tmp: only the bytes the scan wants, into tmp_bytes
inline hipError_t scan_offsets(void *tmp, size_t &tmp_bytes, const uint32_t *sizes, unsigned long long *offsets, size_t n, hipStream_t st)
{
    return rocprim::exclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator(sizes, widen()), offsets, 0ull, n,
                                   rocprim::plus<unsigned long long>(), st);
}

// that scan enqueued, refused where it wants more than the `have` bytes held at tmp
inline int scan_offsets(ochip_ctx *ctx, const char *what, void *tmp, size_t have, const uint32_t *sizes, unsigned long long *offsets, size_t n,
                        hipStream_t st)
{
    size_t need = 0;
    OCHIP_HIP(ctx, scan_offsets(nullptr, need, sizes, offsets, n, st));
    if (need > have)
        return ochip_fail(ctx, OCHIP_EHIP, "%s: the scan of %zu sizes wants %zu bytes, %zu are held", what, n, need, have);
    OCHIP_HIP(ctx, scan_offsets(tmp, need, sizes, offsets, n, st));
    return OCHIP_OK;
}

} // namespace ochip_dfk
