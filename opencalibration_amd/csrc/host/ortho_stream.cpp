// liboc_host.so: the layered render with its source images streamed through a fixed number of device slots, band by band
// (the reference's counterpart: findTileCameras, the LRU image cache and the prefetch thread of generateLayeredGeoTIFF,
// src/ortho/ortho.cpp:1010-1066, 1501-1539).  At create the bands' camera sets come from och_ortho_band_cameras and the
// loads from ortho_residency.hpp; afterwards the caller drives the object by calling, and the object refuses every call
// the plan's order does not allow, so that no band renders from a slot that holds another camera's image.
#include "../../../include/oc_host.h"

#include "../jpeg_decode.hpp"
#include "ortho_residency.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace opencalibration_amd;

namespace
{
thread_local std::string stream_error;

int fail(const std::string &text)
{
    stream_error = "och_ortho_stream: " + text;
    return -1;
}

// upload_jpegs cuts a call into decoder batches of at most this many pixels (host.py's JPEG_LOAD_PIXEL_BUDGET, what
// Graph.load_jpegs decodes at a time) and file bytes (the device route keeps 32-bit byte positions within a batch)
constexpr uint64_t JPEG_BATCH_PIXELS = 1ull << 28, JPEG_BATCH_BYTES = 1ull << 31;
} // namespace

struct och_ortho_stream
{
    const och_graph *g = nullptr;
    ochip_ctx *ctx = nullptr;
    ochip_ortho_mesh *mesh = nullptr;
    std::vector<const och_surface *> surfaces;
    double plan8[8];
    int32_t config4[4];
    int64_t band_rows = 0, height = 0;
    size_t n_bands = 0, n_cams = 0;
    std::vector<int64_t> hw;      // [n_cams][2]
    std::vector<uint8_t> used;    // [n_bands][n_cams]
    std::vector<int32_t> resident; // the slots' state after the sweep planned last
    std::vector<ortho_residency::Load> loads;
    std::vector<size_t> load_off;
    std::vector<std::vector<uint32_t>> band_cams, band_slot; // band k's cameras, ascending, and the slot of each at its render
    // this sweep
    std::vector<uint8_t> uploaded; // per load
    std::vector<size_t> pending;   // per band: planned loads not uploaded yet
    std::vector<uint8_t> marked;   // per band: its mark is recorded behind its last upload
    int64_t rendered = -1;         // the last band whose render has returned
    // the slots: a block of the context's pool (device route) or host memory (CPU route)
    ochip_image_slots *slots = nullptr;
    std::vector<uint8_t> host_slots;
    uint64_t slot_bytes = 0;
    och_jpeg_decoder *decoder = nullptr; // upload_jpegs': made at its first call, on the stream's route

    bool replan()
    {
        std::string error;
        if (!ortho_residency::plan(used.data(), n_bands, n_cams, resident, &loads, &load_off, &error))
        {
            fail(error);
            return false;
        }
        return true;
    }

    // the slot of every camera of every band at its render: the plan replayed from the state `before` it
    void place(std::vector<int32_t> before)
    {
        band_slot.assign(n_bands, {});
        std::vector<int32_t> slot_of(n_cams, -1);
        for (size_t s = 0; s < before.size(); s++)
            if (before[s] != ortho_residency::FREE)
                slot_of[before[s]] = (int32_t)s;
        for (size_t k = 0; k < n_bands; k++)
        {
            for (size_t j = load_off[k]; j < load_off[k + 1]; j++)
            {
                const ortho_residency::Load &l = loads[j];
                if (before[l.slot] != ortho_residency::FREE)
                    slot_of[before[l.slot]] = -1;
                before[l.slot] = l.camera;
                slot_of[l.camera] = l.slot;
            }
            for (uint32_t c : band_cams[k])
                band_slot[k].push_back((uint32_t)slot_of[c]);
        }
    }

    // load j of `band` is in its slot, by copy or by decode: the band's mark goes behind its last one
    int arrived(size_t band, size_t j, const char *who)
    {
        uploaded[j] = 1;
        if (--pending[band] == 0 && slots)
        {
            // the band's event: behind its own uploads, before whatever the caller uploads ahead for the next band
            if (ochip_image_slots_mark(slots, (uint32_t)band) != OCHIP_OK)
                return fail(std::string(who) + ": " + ochip_last_error(ctx));
            marked[band] = 1;
        }
        return 0;
    }

    // the planned load of `camera` for `band` (an index into loads) after upload's checks; false: the refusal is in *why
    bool acceptable(size_t band, uint32_t camera, size_t *load, std::string *why) const
    {
        size_t j = load_off[band];
        while (j < load_off[band + 1] && (uint32_t)loads[j].camera != camera)
            j++;
        if (j == load_off[band + 1])
            return *why = "camera " + std::to_string(camera) + " is no planned load of band " + std::to_string(band), false;
        if (uploaded[j])
            return *why = "camera " + std::to_string(camera) + " of band " + std::to_string(band) + " is uploaded already", false;
        const ortho_residency::Load &l = loads[j];
        // an ahead load's slot is free of bands k - 1 and k, a late load's of band k alone: the band before those has returned
        const int64_t need = (int64_t)band - (l.phase == ortho_residency::AHEAD ? 2 : 1);
        if (rendered < need)
            return *why = "the " + std::string(l.phase == ortho_residency::AHEAD ? "ahead" : "late") + " load of camera " +
                          std::to_string(camera) + " for band " + std::to_string(band) + " waits for render(" + std::to_string(need) +
                          ") to return; the last band rendered is " + std::to_string(rendered),
                   false;
        *load = j;
        return true;
    }

    void start_sweep()
    {
        uploaded.assign(loads.size(), 0);
        pending.assign(n_bands, 0);
        for (size_t k = 0; k < n_bands; k++)
            pending[k] = load_off[k + 1] - load_off[k];
        marked.assign(n_bands, 0);
        rendered = -1;
        if (slots)
            (void)ochip_image_slots_mark(slots, (uint32_t)n_bands); // the sweep's time zero on the copy stream
    }
};

extern "C"
{

int och_ortho_stream_create(const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *mesh, const och_surface *const *surfaces,
                            size_t n, const double *plan8, const int32_t *config4, int64_t band_tile_rows, size_t capacity_images,
                            och_ortho_stream **out)
{
    if (!g || !plan8 || !config4 || !out || (n && !surfaces) || (ctx == nullptr) != (mesh == nullptr))
        return fail("create: bad argument (the device route takes the context and its mesh, the CPU route neither)");
    *out = nullptr;
    if (config4[1] < 1 || band_tile_rows < 1 || capacity_images < 1 || capacity_images > 0x7FFFFFFF ||
        !(plan8[0] >= 0 && plan8[0] <= 2147483647.0 && plan8[1] >= 0 && plan8[1] <= 2147483647.0))
        return fail("create: tile_size, band_tile_rows and capacity_images are at least 1, the plan's size fits an int");
    std::unique_ptr<och_ortho_stream> s(new och_ortho_stream);
    s->g = g, s->ctx = ctx, s->mesh = mesh;
    s->surfaces.assign(surfaces, surfaces + n);
    std::copy(plan8, plan8 + 8, s->plan8);
    std::copy(config4, config4 + 4, s->config4);
    s->band_rows = band_tile_rows * config4[1];
    s->height = (int64_t)plan8[1];
    s->n_bands = (size_t)((s->height + s->band_rows - 1) / s->band_rows);
    s->n_cams = och_ortho_layers_cameras(g, surfaces, n, nullptr, nullptr, nullptr, nullptr);
    std::vector<double> cams(s->n_cams * 28);
    s->hw.resize(s->n_cams * 2);
    och_ortho_layers_cameras(g, surfaces, n, cams.data(), nullptr, nullptr, s->hw.data());
    s->used.assign(s->n_bands * s->n_cams, 0);
    const double raster4[4] = {plan8[3], plan8[6], plan8[2], plan8[7]};
    if (och_ortho_band_cameras(ctx, raster4, (int32_t)plan8[0], s->height, s->band_rows, s->n_cams, cams.data(), s->used.data()) != 0)
        return fail(std::string("create: ") + och_ortho_layers_last_error());
    s->band_cams.assign(s->n_bands, {});
    for (size_t k = 0; k < s->n_bands; k++)
        for (size_t c = 0; c < s->n_cams; c++)
            if (s->used[k * s->n_cams + c])
                s->band_cams[k].push_back((uint32_t)c);
    s->resident.assign(capacity_images, ortho_residency::FREE);
    const std::vector<int32_t> before = s->resident;
    if (!s->replan())
        return -1;
    s->place(before);
    for (size_t c = 0; c < s->n_cams; c++)
        s->slot_bytes = std::max<uint64_t>(s->slot_bytes, (uint64_t)s->hw[2 * c] * (uint64_t)s->hw[2 * c + 1] * 3);
    s->slot_bytes = std::max<uint64_t>(s->slot_bytes, 1);
    if (ctx)
    {
        if (ochip_image_slots_create(ctx, (uint32_t)capacity_images, s->slot_bytes, (uint32_t)s->n_bands + 1, &s->slots) != OCHIP_OK)
            return fail(std::string("create: ") + ochip_last_error(ctx));
    }
    else
        s->host_slots.resize(capacity_images * s->slot_bytes);
    s->start_sweep();
    *out = s.release();
    return 0;
}

void och_ortho_stream_destroy(och_ortho_stream *s)
{
    if (!s)
        return;
    och_jpeg_decoder_destroy(s->decoder);
    ochip_image_slots_destroy(s->slots);
    delete s;
}

size_t och_ortho_stream_num_bands(const och_ortho_stream *s)
{
    return s->n_bands;
}

size_t och_ortho_stream_band_cameras(const och_ortho_stream *s, size_t band, uint32_t *cameras)
{
    if (band >= s->n_bands)
        return 0;
    if (cameras)
        std::copy(s->band_cams[band].begin(), s->band_cams[band].end(), cameras);
    return s->band_cams[band].size();
}

size_t och_ortho_stream_loads(const och_ortho_stream *s, size_t band, int32_t *loads3)
{
    if (band >= s->n_bands)
        return 0;
    const size_t a = s->load_off[band], b = s->load_off[band + 1];
    if (loads3)
        for (size_t j = a; j < b; j++)
            loads3[3 * (j - a)] = s->loads[j].camera, loads3[3 * (j - a) + 1] = s->loads[j].slot, loads3[3 * (j - a) + 2] = s->loads[j].phase;
    return b - a;
}

int och_ortho_stream_upload(och_ortho_stream *s, size_t band, uint32_t camera, const uint8_t *host_bgr)
{
    if (band >= s->n_bands || !host_bgr)
        return fail("upload: band " + std::to_string(band) + " of " + std::to_string(s->n_bands) + ", or no image");
    size_t j = 0;
    std::string why;
    if (!s->acceptable(band, camera, &j, &why))
        return fail("upload: " + why);
    const ortho_residency::Load &l = s->loads[j];
    const uint64_t bytes = (uint64_t)s->hw[2 * camera] * (uint64_t)s->hw[2 * camera + 1] * 3;
    if (s->slots)
    {
        if (ochip_image_slots_upload(s->slots, (uint32_t)l.slot, host_bgr, bytes) != OCHIP_OK)
            return fail(std::string("upload: ") + ochip_last_error(s->ctx));
    }
    else
        std::memcpy(s->host_slots.data() + (size_t)l.slot * s->slot_bytes, host_bgr, bytes);
    return s->arrived(band, j, "upload");
}

// n planned loads of `band` from JPEG files, decoded into their slots by the stream's own decoder.
// Why this needs no event of its own: the decoder's kernels run on the context's compute stream and
// och_jpeg_decoder_decode returns behind its final status read-back and stream wait, so a slot it wrote is complete when
// this function returns; the render of the band runs on that same stream afterwards.  The slot it writes is free: a load
// is accepted only after render(k - 2) / render(k - 1) has returned, render returns behind a stream wait with the band
// written, and that render had waited for its band's mark, which lies behind every copy ever issued into the slot.  The
// copies of the same band still go out on the copy stream and are covered by the band's mark, recorded behind the last
// load whichever way it came.
int och_ortho_stream_upload_jpegs(och_ortho_stream *s, size_t band, size_t n, const uint32_t *cameras, const uint8_t *const *files,
                                  const uint64_t *sizes, ochip_jpeg_file_info *info)
{
    if (band >= s->n_bands)
        return fail("upload_jpegs: band " + std::to_string(band) + " of " + std::to_string(s->n_bands));
    if (n == 0)
        return 0;
    if (!cameras || !files || !sizes)
        return fail("upload_jpegs: a NULL argument");
    // upload's checks for every camera before a byte of a file is read
    std::vector<size_t> load(n);
    std::string why;
    for (size_t i = 0; i < n; i++)
    {
        if (!s->acceptable(band, cameras[i], &load[i], &why))
            return fail("upload_jpegs: " + why);
        if (std::find(cameras, cameras + i, cameras[i]) != cameras + i)
            return fail("upload_jpegs: camera " + std::to_string(cameras[i]) + " appears twice in the call");
        if (!files[i])
            return fail("upload_jpegs: camera " + std::to_string(cameras[i]) + " has no file");
    }
    // the headers, oriented as cv::imread orients the pixels, before anything is launched
    uint8_t *base = s->slots ? reinterpret_cast<uint8_t *>((uintptr_t)ochip_image_slots_address(s->slots, 0)) : s->host_slots.data();
    const uint64_t stride = s->slots && s->resident.size() > 1 ? ochip_image_slots_address(s->slots, 1) - (uint64_t)(uintptr_t)base
                                                               : s->slot_bytes;
    const uint64_t block = (uint64_t)(s->resident.size() - 1) * stride + s->slot_bytes;
    std::vector<uint64_t> offsets(n);
    for (size_t i = 0; i < n; i++)
        offsets[i] = (uint64_t)s->loads[load[i]].slot * stride;
    std::vector<ochip_jpeg_file_info> own(info ? 0 : n);
    info = info ? info : own.data();
    std::vector<ochip_jd::parsed> P;
    why = ochip_jd::plan_batch((int64_t)n, (int64_t)n, files, sizes, true, base, ~0ull, offsets.data(), info, P);
    if (!why.empty())
        return fail("upload_jpegs: " + why);
    static const char *const status_name[3] = {"ok", "unsupported", "corrupt"};
    for (size_t i = 0; i < n; i++)
    {
        const int64_t rows = s->hw[2 * cameras[i]], cols = s->hw[2 * cameras[i] + 1];
        if (info[i].status != OCHIP_JPEG_OK)
            return fail("upload_jpegs: the file of camera " + std::to_string(cameras[i]) + " is " +
                        status_name[info[i].status == OCHIP_JPEG_UNSUPPORTED ? 1 : 2]);
        if (info[i].width != cols || info[i].height != rows)
            return fail("upload_jpegs: the file of camera " + std::to_string(cameras[i]) + " decodes to " + std::to_string(info[i].width) +
                        " x " + std::to_string(info[i].height) + ", the camera's images are " + std::to_string(cols) + " x " +
                        std::to_string(rows));
    }
    if (!s->decoder && och_jpeg_decoder_create(s->ctx, 0, &s->decoder) != 0)
        return fail(std::string("upload_jpegs: ") + och_jpeg_decode_last_error());
    // decoder batches: at most JPEG_BATCH_PIXELS pixels (an image above that alone), the decoder's file count, and file
    // bytes that keep its 32-bit positions
    std::string corrupt;
    for (size_t a = 0; a < n;)
    {
        size_t b = a;
        uint64_t pixels = 0, bytes = 0;
        while (b < n && (b == a || (pixels + (uint64_t)info[b].width * (uint64_t)info[b].height <= JPEG_BATCH_PIXELS &&
                                    bytes + sizes[b] < JPEG_BATCH_BYTES && (int64_t)(b - a) < ochip_jd::MAX_BATCH_FILES)))
        {
            pixels += (uint64_t)info[b].width * (uint64_t)info[b].height, bytes += sizes[b];
            b++;
        }
        if (och_jpeg_decoder_decode(s->decoder, (int64_t)(b - a), files + a, sizes + a, 1, base, block, offsets.data() + a, info + a,
                                    nullptr) != 0)
            return fail(std::string("upload_jpegs: ") + och_jpeg_decode_last_error());
        for (size_t i = a; i < b; i++)
            if (info[i].status != OCHIP_JPEG_OK) // known only now: the load stays pending, upload may still bring its pixels
                corrupt += (corrupt.empty() ? "" : ", ") + std::to_string(cameras[i]);
            else if (s->arrived(band, load[i], "upload_jpegs") != 0)
                return -1;
        a = b;
    }
    if (!corrupt.empty())
        return fail("upload_jpegs: the scan of the file of camera " + corrupt + " is corrupt; its load of band " + std::to_string(band) +
                    " is still pending, the call's other loads are in their slots");
    return 0;
}

int och_ortho_stream_render(och_ortho_stream *s, size_t band, const float *dsm_in, int out_on_device, uint8_t *bgra, uint64_t *ids,
                            float *weight, ochip_color_corr *corr_out, uint64_t corr_capacity, uint64_t *n_corr, uint32_t *knn_out)
{
    if (band >= s->n_bands)
        return fail("render: band " + std::to_string(band) + " of " + std::to_string(s->n_bands));
    if ((int64_t)band != s->rendered + 1)
        return fail("render: bands render in ascending order; band " + std::to_string(band) + " was asked for, band " +
                    std::to_string(s->rendered + 1) + " is next");
    if (s->pending[band])
        return fail("render: " + std::to_string(s->pending[band]) + " planned loads of band " + std::to_string(band) +
                    " are not uploaded");
    const std::vector<uint32_t> &cams = s->band_cams[band];
    std::vector<uint64_t> images(cams.size());
    std::vector<int64_t> hw(2 * cams.size());
    for (size_t i = 0; i < cams.size(); i++)
    {
        const uint32_t slot = s->band_slot[band][i];
        images[i] = s->slots ? ochip_image_slots_address(s->slots, slot)
                             : (uint64_t)(uintptr_t)(s->host_slots.data() + (size_t)slot * s->slot_bytes);
        hw[2 * i] = s->hw[2 * cams[i]], hw[2 * i + 1] = s->hw[2 * cams[i] + 1];
    }
    if (s->slots && s->marked[band] && ochip_image_slots_wait(s->slots, (uint32_t)band, 0) != OCHIP_OK)
        return fail(std::string("render: ") + ochip_last_error(s->ctx));
    const int64_t row0 = (int64_t)band * s->band_rows, rows = std::min(s->band_rows, s->height - row0);
    static const uint32_t none = 0;
    if (och_ortho_layers_render_subset(s->g, s->ctx, s->mesh, s->surfaces.data(), s->surfaces.size(), s->plan8, s->config4, row0,
                                       rows, cams.empty() ? &none : cams.data(), cams.size(), images.data(), hw.data(), dsm_in,
                                       out_on_device, bgra, ids, weight, corr_out, corr_capacity, n_corr, knn_out) != 0)
        return fail(std::string("render: ") + och_ortho_layers_last_error());
    s->rendered = (int64_t)band;
    return 0;
}

int och_ortho_stream_rewind(och_ortho_stream *s)
{
    if (s->rendered + 1 != (int64_t)s->n_bands)
        return fail("rewind: the sweep has rendered " + std::to_string(s->rendered + 1) + " of " + std::to_string(s->n_bands) +
                    " bands");
    // the images the first sweep left in the slots stay: the next sweep loads what is missing from there
    const std::vector<int32_t> before = s->resident;
    if (!s->replan())
        return -1;
    s->place(before);
    s->start_sweep();
    return 0;
}

int och_ortho_stream_upload_end_ms(och_ortho_stream *s, size_t band, double *ms)
{
    if (band >= s->n_bands || !ms || !s->slots || !s->marked[band])
        return fail("upload_end_ms: band " + std::to_string(band) + " has no recorded uploads on a device");
    float f = 0;
    if (ochip_image_slots_elapsed(s->slots, (uint32_t)s->n_bands, (uint32_t)band, &f) != OCHIP_OK)
        return fail(std::string("upload_end_ms: ") + ochip_last_error(s->ctx));
    *ms = f;
    return 0;
}

const char *och_ortho_stream_last_error(void)
{
    return stream_error.c_str();
}

int och_ortho_residency_plan(const uint8_t *used, size_t n_bands, size_t n_cams, size_t capacity, int32_t *resident,
                             size_t *load_off, int32_t *loads3)
{
    if ((n_bands && n_cams && !used) || !resident || !load_off || capacity < 1)
        return fail("residency_plan: bad argument");
    std::vector<int32_t> state(resident, resident + capacity);
    std::vector<ortho_residency::Load> loads;
    std::vector<size_t> off;
    std::string error;
    if (!ortho_residency::plan(used, n_bands, n_cams, state, &loads, &off, &error))
        return fail(error);
    std::copy(off.begin(), off.end(), load_off);
    std::copy(state.begin(), state.end(), resident);
    for (size_t j = 0; j < loads.size() && loads3; j++)
        loads3[3 * j] = loads[j].camera, loads3[3 * j + 1] = loads[j].slot, loads3[3 * j + 2] = loads[j].phase;
    return 0;
}

} // extern "C"
