// The textured OBJ's JPEG texture on the device (the rules: jpeg_encode.hpp).  A feed encodes the MCU
// rows it completes in passes of at most PASS_MCUS MCUs, every pass these launches on the context's stream:
//   jpeg_coefficients  a workgroup of 256 threads takes 4 MCUs of one MCU row: pixels in (16-byte words where the rows allow),
//                      colour conversion, the 2 x 2 chroma average and both DCT passes through LDS - a lane one 8-point
//                      transform - then the quantiser; int16 zigzag coefficients out, 768 bytes an MCU, as 16-byte words.
//   jpeg_lengths       a lane an MCU: its bits.  The DC predictors come from the MCU before in the coefficient array, the
//                      pass's first MCU takes them from the encoder's state words.
//   (rocPRIM)          exclusive scan of the lengths into 64-bit bit offsets
//   jpeg_emit          a lane an MCU: the same walk with a word writer at the MCU's bit offset.  A word that lies inside the
//                      MCU is stored, the two ragged ones at its ends are ORed into the zeroed buffer: the same bytes on
//                      every run, two atomics an MCU and none per symbol.
//   jpeg_tail          one lane: the complete bytes, the new partial byte and predictors into the state words
//   jpeg_count_ff, (rocPRIM), jpeg_stuff   FF bytes per 64-byte chunk, their scan, the scatter with the zeros inserted
// and two copies to page-locked memory: the counts, and as many bytes as the pass before suggests.  A pass writes into one of
// OUT_SLOTS output slots (stuffed bytes, counts, the page-locked blocks, an event); everything ahead of the stuffing is reused
// from pass to pass in stream order.  The host reads a slot when a pass needs it again, at collect or at finish - one wait,
// for the slot's event, recorded behind the pass and so not for what the caller enqueued on the stream since - and fetches
// the rest only when the guess was short.  With OUT_SLOTS passes in flight a feed of up to three passes never waits for
// itself: the mosaic's band loop stays ahead of the device.
#include "ctx.hpp"
#include "jpeg_encode.hpp"
#include "live_handles.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <memory>

namespace
{

using namespace ochip_jp;

constexpr int THREADS = 256, COEF_MCUS = 4, CHUNK = 64;
constexpr int64_t PASS_MCUS = 32768;
constexpr int STATE_WORDS = 8; // Y, Cb, Cr predictors, the partial byte's bits, their count
constexpr int INFO_WORDS = 8;  // complete bytes before stuffing, bytes after it, the partial bits, their count
constexpr int OUT_SLOTS = 4;

struct coef_args
{
    rows_view v;
    geometry g;
    const tables *t;
    int16_t *coef;    // [mcu_rows][mw][384]
    int32_t mcu_row0; // the pass's first MCU row
    int32_t mcu_rows;
    int32_t carry_vec, band_vec; // the rows of that source start on 16 bytes and a pixel has 4
};

__global__ __launch_bounds__(THREADS) void jpeg_coefficients(const coef_args A)
{
    __shared__ int blk[COEF_MCUS][MCU_BLOCKS][72]; // a block's rows 9 apart
    __shared__ uint8_t full[2][COEF_MCUS][256];    // Cb, Cr before the average
    __shared__ uint16_t qd[2][64];
    __shared__ uint8_t zz[64];
    const int t = threadIdx.x;
    if (t < 128)
        qd[t >> 6][t & 63] = A.t->qdiv[t >> 6][t & 63];
    else if (t < 192)
        zz[t - 128] = A.t->zz[t - 128];
    if ((int)blockIdx.y >= A.mcu_rows)
        return;
    const int my = A.mcu_row0 + (int)blockIdx.y, mx0 = (int)blockIdx.x * COEF_MCUS;
    const geometry g = A.g;
    {
        // row r of the 64 x 16 tile, 4 pixels from column lx of MCU m
        const int r = t >> 4, q4 = t & 15, m = q4 >> 2, lx = (q4 & 3) * 4;
        const int64_t X0 = (int64_t)mx0 * 16 + q4 * 4;
        int64_t y = (int64_t)my * 16 + r;
        y = y < g.h ? y : g.h - 1;
        const bool vec = (y < A.v.band_row0 ? A.carry_vec : A.band_vec) != 0;
        uint32_t px[4];
        if (vec && X0 + 3 < g.w)
        {
            const uint4 q = *reinterpret_cast<const uint4 *>(A.v.at(y, X0));
            px[0] = q.x, px[1] = q.y, px[2] = q.z, px[3] = q.w;
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const int64_t x = X0 + j < g.w ? X0 + j : g.w - 1;
                const uint8_t *p = A.v.at(y, x);
                px[j] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            int Y, cb, cr;
            rgb_to_ycc((int)(px[j] & 255), (int)(px[j] >> 8 & 255), (int)(px[j] >> 16 & 255), Y, cb, cr);
            const int c = lx + j;
            blk[m][(r >> 3) * 2 + (c >> 3)][(r & 7) * 9 + (c & 7)] = Y - 128;
            full[0][m][r * 16 + c] = (uint8_t)cb, full[1][m][r * 16 + c] = (uint8_t)cr;
        }
    }
    __syncthreads();
    {
        // chroma sample (cx, cy) of MCU m: the tile's rows already repeat the raster's last row, its columns the last column;
        // below the last averaged row that row repeats (jpeg_encode.hpp, chroma_sample)
        const int m = t >> 6, cy = (t >> 3) & 7, cx = t & 7;
        const int last_cy = (g.h + 1) / 2 - 1, cyg = my * 8 + cy, c = cyg < last_cy ? cyg : last_cy;
        const int at = (2 * c - my * 16) * 16 + 2 * cx; // rows 0 .. 14
        const int bias = (cx & 1) ? 2 : 1;
        const uint8_t *fb = full[0][m], *fr = full[1][m];
        blk[m][4][cy * 9 + cx] = ((fb[at] + fb[at + 1] + fb[at + 16] + fb[at + 17] + bias) >> 2) - 128;
        blk[m][5][cy * 9 + cx] = ((fr[at] + fr[at + 1] + fr[at + 16] + fr[at + 17] + bias) >> 2) - 128;
    }
    __syncthreads();
    const int m = t / 48, rem = t % 48, b = rem >> 3, lane8 = rem & 7; // t < 192: MCU, block, row / column / group of 8
    if (t < 192)
    {
        int *p = &blk[m][b][lane8 * 9];
        int d[8] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
        fdct8<true>(d);
        p[0] = d[0], p[1] = d[1], p[2] = d[2], p[3] = d[3], p[4] = d[4], p[5] = d[5], p[6] = d[6], p[7] = d[7];
    }
    __syncthreads();
    if (t < 192)
    {
        int *p = &blk[m][b][lane8];
        int d[8] = {p[0], p[9], p[18], p[27], p[36], p[45], p[54], p[63]};
        fdct8<false>(d);
        p[0] = d[0], p[9] = d[1], p[18] = d[2], p[27] = d[3], p[36] = d[4], p[45] = d[5], p[54] = d[6], p[63] = d[7];
    }
    __syncthreads();
    const int mx = mx0 + m;
    if (t >= 192 || mx >= g.mw)
        return;
    const int comp = b < 4 ? 0 : 1, k0 = lane8 * 8;
    const bool real = b >= 4 || luma_block_real(g, mx, my, b);
    uint32_t w[4] = {0, 0, 0, 0};
    if (real)
    {
#pragma unroll
        for (int i = 0; i < 8; i++)
        {
            const int nat = zz[k0 + i];
            const int v = quantise(blk[m][b][(nat >> 3) * 9 + (nat & 7)], qd[comp][nat]);
            w[i >> 1] |= ((uint32_t)v & 0xFFFFu) << ((i & 1) * 16);
        }
    }
    else if (k0 == 0)
    {
        // a dummy block: the DC of the block coded before it in this MCU, which may be a dummy itself; block 0 is real
        int s = b - 1;
        while (s > 0 && !luma_block_real(g, mx, my, s))
            s--;
        w[0] = (uint32_t)quantise(blk[m][s][0], qd[0][0]) & 0xFFFFu;
    }
    const size_t at = ((size_t)blockIdx.y * (size_t)g.mw + (size_t)mx) * MCU_COEFS + (size_t)b * 64 + (size_t)k0;
    *reinterpret_cast<uint4 *>(A.coef + at) = make_uint4(w[0], w[1], w[2], w[3]);
}

// Rows of a band behind the carried rows: [rows][w] pixels of `stride` bytes to 4-byte pixels
__global__ __launch_bounds__(THREADS) void jpeg_keep_rows(const uint8_t *src, int stride, size_t pixels, uchar4 *dst)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= pixels)
        return;
    const uint8_t *p = src + i * (size_t)stride;
    dst[i] = make_uchar4(p[0], p[1], p[2], 255);
}

// The Huffman tables in LDS: [0, 24) the DC entries, [24, 536) the AC entries
__device__ void load_huffman(const tables *t, uint32_t *lds)
{
    for (int i = threadIdx.x; i < 24 + 512; i += THREADS)
        lds[i] = i < 24 ? t->dc[i / 12][i % 12] : t->ac[(i - 24) >> 8][(i - 24) & 255];
}

// The entropy coder over MCU m of the pass into a sink; state: the predictors ahead of the pass
template <class Sink> __device__ void code_mcu(Sink &sink, const int16_t *coef, size_t m, const int32_t *state, const uint32_t *huff)
{
    const int16_t *mcu = coef + m * MCU_COEFS;
    int pred[3];
    if (m == 0)
        pred[0] = state[0], pred[1] = state[1], pred[2] = state[2];
    else
        pred[0] = mcu[-MCU_COEFS + 192], pred[1] = mcu[-MCU_COEFS + 256], pred[2] = mcu[-MCU_COEFS + 320];
    int prev_y = pred[0];
    for (int b = 0; b < MCU_BLOCKS; b++)
    {
        const int comp = b < 4 ? 0 : 1;
        block_coder<Sink> coder(sink, huff + comp * 12, huff + 24 + comp * 256);
        const uint4 *p = reinterpret_cast<const uint4 *>(mcu + b * 64);
        for (int wd = 0; wd < 8; wd++)
        {
            const uint4 q = p[wd];
            const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const int lo = (int16_t)(ws[j] & 0xFFFFu), hi = (int16_t)(ws[j] >> 16);
                if (wd == 0 && j == 0)
                {
                    coder.dc(lo - (b < 4 ? prev_y : b == 4 ? pred[1] : pred[2]));
                    if (b < 4)
                        prev_y = lo;
                }
                else
                    coder.ac(lo);
                coder.ac(hi);
            }
        }
        coder.end();
    }
}

__global__ __launch_bounds__(THREADS) void jpeg_lengths(const int16_t *coef, size_t n, const int32_t *state, const tables *t, uint32_t *bits)
{
    __shared__ uint32_t huff[24 + 512];
    load_huffman(t, huff);
    __syncthreads();
    const size_t m = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (m > n)
        return;
    bit_counter c;
    if (m < n)
        code_mcu(c, coef, m, state, huff);
    bits[m] = c.bits; // bits[n] = 0: the scan's last output is the total
}

// Bits from `pos` on into 32-bit words whose bytes lie in stream order.  A word the MCU fills alone is stored; the first
// word when the MCU starts inside it and the last partial one are ORed into the zeroed buffer.
struct word_writer
{
    uint32_t *words;
    size_t wi;
    uint64_t acc;
    int n;
    bool shared_first;
    __device__ void put(uint32_t bits, int len)
    {
        acc = (acc << len) | bits, n += len;
        if (n >= 32)
        {
            const uint32_t w = __builtin_bswap32((uint32_t)(acc >> (n - 32)));
            if (shared_first)
                atomicOr(&words[wi], w);
            else
                words[wi] = w;
            shared_first = false;
            wi++, n -= 32;
            acc &= (1ull << n) - 1;
        }
    }
    __device__ void flush()
    {
        if (n > 0)
            atomicOr(&words[wi], __builtin_bswap32((uint32_t)(acc << (32 - n))));
    }
};

__global__ __launch_bounds__(THREADS) void jpeg_emit(const int16_t *coef, size_t n, const int32_t *state, const tables *t,
                                                      const unsigned long long *offsets, uint32_t *words, size_t n_words)
{
    __shared__ uint32_t huff[24 + 512];
    load_huffman(t, huff);
    __syncthreads();
    const size_t m = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= n)
        return;
    const int carried = state[4];
    const uint64_t pos = (uint64_t)carried + offsets[m], end = (uint64_t)carried + offsets[m + 1];
    if ((end + 31) / 32 > n_words) // cannot happen with lengths within MCU_MAX_BYTES; never write beyond the buffer
        return;
    word_writer w;
    w.words = words, w.wi = (size_t)(pos >> 5);
    if (m == 0) // the bits carried from the pass before start the stream: this lane owns them
        w.acc = (uint32_t)state[3], w.n = carried, w.shared_first = false;
    else
        w.acc = 0, w.n = (int)(pos & 31), w.shared_first = w.n != 0;
    code_mcu(w, coef, m, state, huff);
    w.flush();
}

__global__ void jpeg_tail(const int16_t *coef, size_t n, const unsigned long long *offsets, const uint32_t *words, int32_t *state,
                          unsigned long long *info)
{
    if (threadIdx.x || blockIdx.x)
        return;
    const uint64_t total = (uint64_t)state[4] + offsets[n], complete = total >> 3;
    const int nb = (int)(total & 7);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    const int partial = nb ? bytes[complete] >> (8 - nb) : 0;
    const int16_t *last = coef + (n - 1) * MCU_COEFS;
    state[0] = last[192], state[1] = last[256], state[2] = last[320];
    state[3] = partial, state[4] = nb;
    info[0] = complete, info[2] = (unsigned long long)partial, info[3] = (unsigned long long)nb;
}

// chunk i: the FF bytes among the complete bytes [64 i, 64 i + 64); counts[chunks] = 0
__global__ __launch_bounds__(THREADS) void jpeg_count_ff(const uint32_t *words, const unsigned long long *info, size_t chunks,
                                                          uint32_t *counts)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i > chunks)
        return;
    const uint64_t complete = info[0], base = (uint64_t)i * CHUNK;
    uint32_t c = 0;
    if (i < chunks && base < complete)
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(words) + i * (CHUNK / 16);
        for (int wd = 0; wd < CHUNK / 16; wd++)
        {
            const uint4 q = p[wd];
            const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 4; k++)
                    c += (base + (uint64_t)(wd * 16 + j * 4 + k) < complete && ((ws[j] >> (8 * k)) & 255u) == 255u) ? 1u : 0u;
        }
    }
    counts[i] = c;
}

__global__ __launch_bounds__(THREADS) void jpeg_stuff(const uint32_t *words, unsigned long long *info, size_t chunks,
                                                       const unsigned long long *ff_before, uint8_t *out, uint64_t out_cap)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= chunks)
        return;
    const uint64_t complete = info[0], base = (uint64_t)i * CHUNK;
    if (i == 0)
        info[1] = complete + ff_before[chunks];
    if (base >= complete)
        return;
    uint64_t o = base + ff_before[i];
    const uint4 *p = reinterpret_cast<const uint4 *>(words) + i * (CHUNK / 16);
    for (int wd = 0; wd < CHUNK / 16; wd++)
    {
        const uint4 q = p[wd];
        const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                const uint32_t byte = (ws[j] >> (8 * k)) & 255u;
                if (base + (uint64_t)(wd * 16 + j * 4 + k) < complete && o + 2 <= out_cap)
                {
                    out[o++] = (uint8_t)byte;
                    if (byte == 255u)
                        out[o++] = 0;
                }
            }
    }
}

struct widen
{
    __host__ __device__ unsigned long long operator()(uint32_t v) const
    {
        return v;
    }
};

ochip::live_set<ochip_jpeg> g_live; // the encoders that exist

size_t blocks_of(size_t n)
{
    return (n + THREADS - 1) / THREADS;
}

} // namespace

struct ochip_jpeg
{
    ochip_ctx *ctx = nullptr;
    geometry g;
    tables t;
    progress P;
    byte_stream out;
    ochip::dev_blocks mem; // everything on the device, held until destroy
    tables *t_dev = nullptr;
    int32_t *state = nullptr; // [STATE_WORDS]
    uint8_t *carry = nullptr; // [15][w] 4-byte pixels
    // a feed is cut into bands of pass_rows * 16 rows; with the carried rows and the raster's ragged end a band completes up
    // to max_rows MCU rows, one pass
    int64_t pass_rows = 0, max_rows = 0, pass_mcus = 0;
    size_t word_bytes = 0, chunks_cap = 0, stuffed_cap = 0, scan_bytes = 0, upload_bytes = 0;
    int16_t *coef = nullptr;
    uint32_t *bits = nullptr;             // [pass_mcus + 1]
    unsigned long long *offsets = nullptr; // [pass_mcus + 1]
    uint32_t *words = nullptr;            // the pass's bits before stuffing
    uint32_t *ff_count = nullptr;         // [chunks_cap + 1]
    unsigned long long *ff_before = nullptr;
    void *scan_tmp = nullptr;
    uint8_t *upload = nullptr; // a host band's copy, made at the first host feed
    void *pin_upload = nullptr; // a page-locked block of the context's pool
    hipEvent_t fed = nullptr;   // recorded behind a feed's last launch
    bool in_flight = false;     // ... and not waited for yet
    // where a pass leaves its bytes; pass k uses slot k % OUT_SLOTS
    struct out_slot
    {
        uint8_t *stuffed = nullptr;
        unsigned long long *info = nullptr;           // [INFO_WORDS]
        void *pin_info = nullptr, *pin_bytes = nullptr; // page-locked blocks of the context's pool
        size_t pin_bytes_cap = 0;
        hipEvent_t done = nullptr; // recorded behind the pass's copies
        bool pending = false;      // the pass's bytes have not been read yet
        int64_t mcus = 0;
        size_t guess = 0;
    } slot[OUT_SLOTS];
    uint64_t passes = 0, passes_read = 0;
    double bytes_per_mcu = 96;
    uint32_t partial = 0; // the stream's last partial byte after the last pass read
    int partial_bits = 0;
};

namespace
{

// the events and the page-locked blocks (what was never made is NULL)
void release_host_side(ochip_jpeg *e)
{
    if (e->fed)
        (void)hipEventDestroy(e->fed);
    ochip_host_free(e->ctx, e->pin_upload);
    for (ochip_jpeg::out_slot &o : e->slot)
    {
        if (o.done)
            (void)hipEventDestroy(o.done);
        ochip_host_free(e->ctx, o.pin_info);
        ochip_host_free(e->ctx, o.pin_bytes);
    }
}

int launched(ochip_ctx *ctx, const char *what)
{
    return hipGetLastError() == hipSuccess ? OCHIP_OK : ochip_fail(ctx, OCHIP_EHIP, "%s launch failed", what);
}

// The oldest pending pass's bytes into the host stream: the one wait
int drain_oldest(ochip_jpeg *e)
{
    ochip_ctx *ctx = e->ctx;
    ochip_jpeg::out_slot &o = e->slot[e->passes_read % OUT_SLOTS];
    if (e->passes_read == e->passes || !o.pending)
        return OCHIP_OK;
    o.pending = false, e->passes_read++;
    OCHIP_HIP(ctx, hipEventSynchronize(o.done));
    const unsigned long long *info = static_cast<const unsigned long long *>(o.pin_info);
    const size_t count = (size_t)info[1];
    if (info[0] > (unsigned long long)o.mcus * MCU_MAX_BYTES + 1 || count > e->stuffed_cap || info[3] > 7)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_jpeg: %llu bytes (%llu before stuffing) from %lld MCUs", info[1], info[0],
                          (long long)o.mcus);
    const size_t have = count < o.guess ? count : o.guess;
    const uint8_t *src = static_cast<const uint8_t *>(o.pin_bytes);
    e->out.bytes.insert(e->out.bytes.end(), src, src + have);
    if (count > have) // the guess was short: the rest directly
    {
        const size_t at = e->out.bytes.size();
        e->out.bytes.resize(at + (count - have));
        OCHIP_HIP(ctx, hipMemcpy(e->out.bytes.data() + at, o.stuffed + have, count - have, hipMemcpyDeviceToHost));
    }
    e->bytes_per_mcu = (double)count / (double)o.mcus;
    e->partial = (uint32_t)info[2], e->partial_bits = (int)info[3];
    return OCHIP_OK;
}

// Every pending pass, oldest first, and the feed's last launch
int drain(ochip_jpeg *e)
{
    while (e->passes_read < e->passes)
        OCHIP_TRY(drain_oldest(e));
    if (e->in_flight)
    {
        e->in_flight = false;
        OCHIP_HIP(e->ctx, hipEventSynchronize(e->fed));
    }
    return OCHIP_OK;
}

// One pass: the MCU rows [mcu_row0, mcu_row0 + mcu_rows) from the view, enqueued
int encode_pass(ochip_jpeg *e, const rows_view &v, int carry_vec, int band_vec, int64_t mcu_row0, int64_t mcu_rows)
{
    ochip_ctx *ctx = e->ctx;
    const size_t n = (size_t)mcu_rows * (size_t)e->g.mw;
    if (mcu_rows < 1 || mcu_rows > e->max_rows || n > (size_t)e->pass_mcus)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_feed: a pass of %lld MCU rows, at most %lld", (long long)mcu_rows,
                          (long long)e->max_rows);
    const size_t word_bytes = (n * MCU_MAX_BYTES + 1 + 63) / 64 * 64; // whole chunks; <= e->word_bytes
    const size_t chunks = word_bytes / CHUNK;                          // <= e->chunks_cap
    hipStream_t st = ctx->stream;
    ochip_jpeg::out_slot &o = e->slot[e->passes % OUT_SLOTS];
    while (o.pending) // the slot's last pass has not been read: OUT_SLOTS passes back
        OCHIP_TRY(drain_oldest(e));
    OCHIP_HIP(ctx, hipMemsetAsync(e->words, 0, word_bytes, st));
    coef_args A{};
    A.v = v, A.g = e->g, A.t = e->t_dev, A.coef = e->coef, A.mcu_row0 = (int32_t)mcu_row0, A.mcu_rows = (int32_t)mcu_rows;
    A.carry_vec = carry_vec, A.band_vec = band_vec;
    hipLaunchKernelGGL(jpeg_coefficients, dim3((uint32_t)((e->g.mw + COEF_MCUS - 1) / COEF_MCUS), (uint32_t)mcu_rows), dim3(THREADS), 0, st, A);
    OCHIP_TRY(launched(ctx, "jpeg_coefficients"));
    hipLaunchKernelGGL(jpeg_lengths, dim3((uint32_t)blocks_of(n + 1)), dim3(THREADS), 0, st, e->coef, n, e->state, e->t_dev, e->bits);
    OCHIP_TRY(launched(ctx, "jpeg_lengths"));
    size_t need = 0;
    auto bits64 = rocprim::make_transform_iterator(e->bits, widen());
    OCHIP_HIP(ctx, rocprim::exclusive_scan(nullptr, need, bits64, e->offsets, 0ull, n + 1, rocprim::plus<unsigned long long>(), st));
    if (need > e->scan_bytes)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_jpeg_feed: the scan of %zu lengths wants %zu bytes, %zu are held", n + 1, need, e->scan_bytes);
    OCHIP_HIP(ctx, rocprim::exclusive_scan(e->scan_tmp, need, bits64, e->offsets, 0ull, n + 1, rocprim::plus<unsigned long long>(), st));
    hipLaunchKernelGGL(jpeg_emit, dim3((uint32_t)blocks_of(n)), dim3(THREADS), 0, st, e->coef, n, e->state, e->t_dev, e->offsets, e->words,
                       word_bytes / 4);
    OCHIP_TRY(launched(ctx, "jpeg_emit"));
    hipLaunchKernelGGL(jpeg_tail, dim3(1), dim3(64), 0, st, e->coef, n, e->offsets, e->words, e->state, o.info);
    OCHIP_TRY(launched(ctx, "jpeg_tail"));
    hipLaunchKernelGGL(jpeg_count_ff, dim3((uint32_t)blocks_of(chunks + 1)), dim3(THREADS), 0, st, e->words, o.info, chunks, e->ff_count);
    OCHIP_TRY(launched(ctx, "jpeg_count_ff"));
    auto ff64 = rocprim::make_transform_iterator(e->ff_count, widen());
    OCHIP_HIP(ctx, rocprim::exclusive_scan(nullptr, need, ff64, e->ff_before, 0ull, chunks + 1, rocprim::plus<unsigned long long>(), st));
    if (need > e->scan_bytes)
        return ochip_fail(ctx, OCHIP_EHIP, "ochip_jpeg_feed: the scan of %zu chunks wants %zu bytes, %zu are held", chunks + 1, need, e->scan_bytes);
    OCHIP_HIP(ctx, rocprim::exclusive_scan(e->scan_tmp, need, ff64, e->ff_before, 0ull, chunks + 1, rocprim::plus<unsigned long long>(), st));
    hipLaunchKernelGGL(jpeg_stuff, dim3((uint32_t)blocks_of(chunks)), dim3(THREADS), 0, st, e->words, o.info, chunks, e->ff_before, o.stuffed,
                       (uint64_t)e->stuffed_cap);
    OCHIP_TRY(launched(ctx, "jpeg_stuff"));
    // the counts, and the bytes the pass before suggests
    size_t guess = (size_t)(e->bytes_per_mcu * 1.25 * (double)n) + 4096;
    const size_t bound = 2 * (n * MCU_MAX_BYTES + 1);
    guess = guess < bound ? guess : bound;
    if (guess > o.pin_bytes_cap)
    {
        ochip_host_free(ctx, o.pin_bytes);
        o.pin_bytes = nullptr, o.pin_bytes_cap = 0;
        OCHIP_TRY(ochip_host_alloc(ctx, guess + guess / 4, &o.pin_bytes));
        o.pin_bytes_cap = guess + guess / 4;
    }
    OCHIP_HIP(ctx, hipMemcpyAsync(o.pin_info, o.info, INFO_WORDS * 8, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, hipMemcpyAsync(o.pin_bytes, o.stuffed, guess, hipMemcpyDeviceToHost, st));
    OCHIP_HIP(ctx, hipEventRecord(o.done, st));
    o.pending = true, o.mcus = (int64_t)n, o.guess = guess;
    e->passes++;
    return OCHIP_OK;
}

// A band of at most pass_rows * 16 rows
int feed_rows(ochip_jpeg *e, int64_t row0, int64_t rows, const uint8_t *pixels, int stride, bool on_device)
{
    ochip_ctx *ctx = e->ctx;
    progress::plan p;
    const std::string refusal = e->P.feed(row0, rows, p);
    if (!refusal.empty())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_feed: %s", refusal.c_str());
    const size_t w = (size_t)e->g.w, band_bytes = (size_t)rows * w * (size_t)stride;
    // the upload block is in use until what read it last has run
    if (!on_device)
        OCHIP_TRY(drain(e));
    const uint8_t *band = pixels;
    if (!on_device)
    {
        if (!e->upload)
        {
            OCHIP_TRY(e->mem.alloc(&e->upload, e->upload_bytes));
            OCHIP_TRY(ochip_host_alloc(ctx, e->upload_bytes, &e->pin_upload));
        }
        if (band_bytes > e->upload_bytes)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_feed: a band of %zu bytes, the block holds %zu", band_bytes, e->upload_bytes);
        std::memcpy(e->pin_upload, pixels, band_bytes);
        OCHIP_HIP(ctx, hipMemcpyAsync(e->upload, e->pin_upload, band_bytes, hipMemcpyHostToDevice, ctx->stream));
        band = e->upload;
    }
    if (p.mcu_rows > 0)
    {
        rows_view v;
        v.carry = e->carry, v.carry_row0 = p.mcu_row0 * 16, v.carry_stride = 4;
        v.band = band, v.band_row0 = row0, v.band_stride = stride, v.w = e->g.w;
        const int carry_vec = w % 4 == 0 && (uintptr_t)e->carry % 16 == 0;
        const int band_vec = stride == 4 && w % 4 == 0 && (uintptr_t)band % 16 == 0;
        OCHIP_TRY(encode_pass(e, v, carry_vec, band_vec, p.mcu_row0, p.mcu_rows));
    }
    if (p.keep_rows > 0)
    {
        if (p.keep_at + p.keep_rows > 15)
            return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_feed: %lld rows to keep behind row %lld", (long long)p.keep_rows, (long long)p.keep_at);
        const size_t pixels_kept = (size_t)p.keep_rows * w;
        hipLaunchKernelGGL(jpeg_keep_rows, dim3((uint32_t)blocks_of(pixels_kept)), dim3(THREADS), 0, ctx->stream,
                           band + (size_t)(p.keep_from - row0) * w * (size_t)stride, stride, pixels_kept,
                           reinterpret_cast<uchar4 *>(e->carry) + (size_t)p.keep_at * w);
        OCHIP_TRY(launched(ctx, "jpeg_keep_rows"));
    }
    OCHIP_HIP(ctx, hipEventRecord(e->fed, ctx->stream));
    e->in_flight = true;
    return OCHIP_OK;
}

} // namespace

extern "C"
{

int ochip_jpeg_create(ochip_ctx *ctx, int64_t width, int64_t height, int quality, ochip_jpeg **out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (!out)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_create: out is NULL");
    *out = nullptr;
    const std::string refusal = refuse_create(width, height, quality);
    if (!refusal.empty())
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_create: %s", refusal.c_str());
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<ochip_jpeg> e(new ochip_jpeg);
    e->ctx = ctx, e->g = make_geometry(width, height);
    build_tables(quality, e->t);
    e->P.height = height;
    e->mem.ctx = ctx, e->mem.what = "ochip_jpeg";
    const int64_t per_pass = PASS_MCUS / e->g.mw > 0 ? PASS_MCUS / e->g.mw : 1;
    e->pass_rows = per_pass < e->g.mh ? per_pass : e->g.mh;
    e->max_rows = e->pass_rows + 1 < e->g.mh ? e->pass_rows + 1 : e->g.mh;
    e->pass_mcus = e->max_rows * e->g.mw;
    const size_t n = (size_t)e->pass_mcus;
    e->word_bytes = (n * MCU_MAX_BYTES + 1 + 63) / 64 * 64;
    e->chunks_cap = e->word_bytes / CHUNK;
    e->stuffed_cap = 2 * e->word_bytes + 16;
    e->upload_bytes = (size_t)e->pass_rows * 16 * (size_t)width * 4;
    // the temporary storage of the larger of the two scans
    size_t a = 0, b = 0;
    unsigned long long *none = nullptr;
    OCHIP_HIP(ctx, rocprim::exclusive_scan(nullptr, a, rocprim::make_transform_iterator((uint32_t *)nullptr, widen()), none, 0ull, n + 1,
                                           rocprim::plus<unsigned long long>(), (hipStream_t)ctx->stream));
    OCHIP_HIP(ctx, rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator((uint32_t *)nullptr, widen()), none, 0ull,
                                           e->chunks_cap + 1, rocprim::plus<unsigned long long>(), (hipStream_t)ctx->stream));
    e->scan_bytes = (a > b ? a : b) + 256;
    int rc = e->mem.upload(&e->t_dev, &e->t, 1, ochip::copy_mode::blocking);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->state, STATE_WORDS);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->carry, (size_t)15 * (size_t)width * 4);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->coef, n * MCU_COEFS);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->bits, n + 1);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->offsets, n + 1);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->words, e->word_bytes / 4);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->ff_count, e->chunks_cap + 1);
    if (rc == OCHIP_OK)
        rc = e->mem.alloc(&e->ff_before, e->chunks_cap + 1);
    if (rc == OCHIP_OK)
        rc = (e->scan_tmp = e->mem.get(e->scan_bytes)) ? OCHIP_OK : OCHIP_ENOMEM;
    for (int k = 0; k < OUT_SLOTS && rc == OCHIP_OK; k++)
    {
        ochip_jpeg::out_slot &o = e->slot[k];
        rc = e->mem.alloc(&o.stuffed, e->stuffed_cap);
        if (rc == OCHIP_OK)
            rc = e->mem.alloc(&o.info, INFO_WORDS);
        if (rc == OCHIP_OK)
            rc = ochip_host_alloc(ctx, INFO_WORDS * 8, &o.pin_info);
        if (rc == OCHIP_OK && hipEventCreateWithFlags(&o.done, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess)
            rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_jpeg_create: hipEventCreateWithFlags failed");
    }
    if (rc == OCHIP_OK && hipEventCreateWithFlags(&e->fed, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess)
        rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_jpeg_create: hipEventCreateWithFlags failed");
    if (rc == OCHIP_OK && hipMemsetAsync(e->state, 0, STATE_WORDS * 4, ctx->stream) != hipSuccess)
        rc = ochip_fail(ctx, OCHIP_EHIP, "ochip_jpeg_create: hipMemsetAsync failed");
    if (rc != OCHIP_OK)
    {
        if (ctx->stream.opened())
            (void)ochip_stream_wait(ctx, ctx->stream);
        release_host_side(e.get());
        e->mem.release();
        return rc;
    }
    append_header(e->out.bytes, e->g, e->t);
    g_live.add(e.get());
    *out = e.release();
    return OCHIP_OK;
}

int ochip_jpeg_feed(ochip_jpeg *e, int64_t row0, int64_t rows, const void *pixels, int pixel_stride, int on_device)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_jpeg_feed: not a live ochip_jpeg object");
    ochip_ctx *ctx = e->ctx;
    if (!pixels)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_feed: the band is NULL");
    if (pixel_stride != 3 && pixel_stride != 4)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_jpeg_feed: a pixel of %d bytes, it has 3 or 4", pixel_stride);
    {
        progress probe = e->P; // the whole band is refused or taken
        progress::plan p;
        const std::string refusal = probe.feed(row0, rows, p);
        if (!refusal.empty())
            return ochip_fail(ctx, e->P.finished ? OCHIP_ESTATE : OCHIP_EINVAL, "ochip_jpeg_feed: %s", refusal.c_str());
    }
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t step = e->pass_rows * 16;
    for (int64_t at = 0; at < rows; at += step)
        OCHIP_TRY(feed_rows(e, row0 + at, rows - at < step ? rows - at : step,
                            static_cast<const uint8_t *>(pixels) + (size_t)at * (size_t)e->g.w * (size_t)pixel_stride, pixel_stride,
                            on_device != 0));
    return OCHIP_OK;
}

int64_t ochip_jpeg_pending(ochip_jpeg *e)
{
    if (!g_live.has(e))
        return 0;
    (void)drain(e);
    return (int64_t)e->out.bytes.size();
}

int ochip_jpeg_collect(ochip_jpeg *e, uint8_t *buf, uint64_t cap, uint64_t *n)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_jpeg_collect: not a live ochip_jpeg object");
    if (!n)
        return ochip_fail(e->ctx, OCHIP_EINVAL, "ochip_jpeg_collect: no count");
    *n = 0;
    OCHIP_TRY(drain(e));
    const std::string refusal = e->out.collect(buf, cap, n);
    return refusal.empty() ? OCHIP_OK : ochip_fail(e->ctx, OCHIP_EINVAL, "ochip_jpeg_collect: %s", refusal.c_str());
}

int ochip_jpeg_finish(ochip_jpeg *e)
{
    if (!g_live.has(e))
        return ochip_fail(nullptr, OCHIP_EINVAL, "ochip_jpeg_finish: not a live ochip_jpeg object");
    {
        progress probe = e->P;
        const std::string refusal = probe.finish();
        if (!refusal.empty())
            return ochip_fail(e->ctx, OCHIP_ESTATE, "ochip_jpeg_finish: %s", refusal.c_str());
    }
    OCHIP_TRY(drain(e));
    (void)e->P.finish();
    append_tail(e->out.bytes, e->partial, e->partial_bits);
    return OCHIP_OK;
}

void ochip_jpeg_destroy(ochip_jpeg *e)
{
    if (!g_live.remove(e))
        return;
    if (e->ctx->stream.opened()) // nothing may still touch the blocks when they go back to the pools
        (void)ochip_stream_wait(e->ctx, e->ctx->stream);
    release_host_side(e);
    e->mem.release();
    delete e;
}

} // extern "C"
