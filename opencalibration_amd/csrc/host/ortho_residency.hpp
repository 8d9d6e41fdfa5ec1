// liboc_host.so: which source images a streamed layered render keeps on the device, and when each one is loaded.
// Pure logic: the bands' camera sets are known before the first band renders (och_ortho_band_cameras), so the plan is made
// up front and the stream object (ortho_stream.cpp) only enforces it.  The reference keeps an LRU cache of num_layers * 10
// images and loads on a miss (src/ortho/ortho.cpp:1010-1066); with every set known, Belady's choice replaces the LRU.
//
// The rule.  C image slots; band k reads the cameras S_k; bands render in ascending order.  The plan walks the bands in
// that order over the slots' state (the camera each slot holds, or none), which a first sweep hands to the next one.
//   - A camera of S_k that is resident is not loaded again.
//   - The missing cameras of S_k are taken in ascending camera order, one load each.
//   - An AHEAD load of band k is issued while band k - 1 renders: it may take a free slot, or a slot whose camera is in
//     neither S_{k-1} nor S_k (S_{-1} is empty: nothing renders before a sweep's first band).
//   - A LATE load of band k is issued after band k - 1 has finished: it may take any slot whose camera is not in S_k.
//   - A load is ahead while an ahead-permitted slot exists, late otherwise.
//   - Slot choice among the permitted ones: a free slot first, the lowest index; otherwise the slot whose camera's next use
//     (the first band after k that reads it) is farthest away, a camera no later band reads counting as farthest; ties go
//     to the lowest slot.
//   - |S_k| > C is refused, naming the band, |S_k| and C.
// |S_k| <= C guarantees a late-permitted slot: before a load fewer than |S_k| slots hold cameras of S_k.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace opencalibration_amd
{
namespace ortho_residency
{

constexpr int32_t FREE = -1;
enum Phase : int32_t
{
    AHEAD = 0,
    LATE = 1
};

struct Load
{
    int32_t camera, slot, phase;
};

// used [n_bands][n_cams] bytes (non-zero: the band reads the camera); resident [capacity]: the camera each slot holds
// (FREE: none), updated to the state after the last band.  loads / load_off (n_bands + 1 offsets into loads): every band's
// loads in issue order.  false + error when a band needs more than `capacity` images or `resident` is malformed.
inline bool plan(const uint8_t *used, size_t n_bands, size_t n_cams, std::vector<int32_t> &resident, std::vector<Load> *loads,
                 std::vector<size_t> *load_off, std::string *error)
{
    const size_t C = resident.size();
    loads->clear();
    load_off->assign(1, 0);
    std::vector<int32_t> slot_of(n_cams, -1);
    for (size_t s = 0; s < C; s++)
    {
        const int32_t c = resident[s];
        if (c == FREE)
            continue;
        if (c < 0 || (size_t)c >= n_cams || slot_of[c] != -1)
        {
            *error = "residency plan: slot " + std::to_string(s) + " holds camera " + std::to_string(c) +
                     ", which is out of range or held twice";
            return false;
        }
        slot_of[c] = (int32_t)s;
    }
    // next_use[k][c]: the first band >= k that reads camera c, n_bands when none does
    std::vector<uint32_t> next_use((n_bands + 1) * n_cams, (uint32_t)n_bands);
    for (size_t k = n_bands; k-- > 0;)
        for (size_t c = 0; c < n_cams; c++)
            next_use[k * n_cams + c] = used[k * n_cams + c] ? (uint32_t)k : next_use[(k + 1) * n_cams + c];
    for (size_t k = 0; k < n_bands; k++)
    {
        const uint8_t *cur = used + k * n_cams, *prev = k ? used + (k - 1) * n_cams : nullptr;
        size_t size = 0;
        for (size_t c = 0; c < n_cams; c++)
            size += cur[c] != 0;
        if (size > C)
        {
            *error = "residency plan: band " + std::to_string(k) + " reads " + std::to_string(size) + " images, the capacity is " +
                     std::to_string(C);
            return false;
        }
        for (size_t c = 0; c < n_cams; c++)
        {
            if (!cur[c] || slot_of[c] != -1)
                continue;
            // the best permitted slot of each kind: free, ahead-permitted, late-permitted
            int32_t free_slot = -1, ahead = -1, late = -1;
            uint32_t ahead_use = 0, late_use = 0;
            for (size_t s = 0; s < C; s++)
            {
                const int32_t h = resident[s];
                if (h == FREE)
                {
                    if (free_slot < 0)
                        free_slot = (int32_t)s;
                    continue;
                }
                if (cur[h])
                    continue;
                const uint32_t use = next_use[(k + 1) * n_cams + h];
                if (late < 0 || use > late_use)
                    late = (int32_t)s, late_use = use;
                if (!(prev && prev[h]) && (ahead < 0 || use > ahead_use))
                    ahead = (int32_t)s, ahead_use = use;
            }
            const int32_t slot = free_slot >= 0 ? free_slot : ahead >= 0 ? ahead : late;
            const int32_t phase = free_slot >= 0 || ahead >= 0 ? AHEAD : LATE;
            if (resident[slot] != FREE)
                slot_of[resident[slot]] = -1;
            resident[slot] = (int32_t)c;
            slot_of[c] = slot;
            loads->push_back(Load{(int32_t)c, slot, phase});
        }
        load_off->push_back(loads->size());
    }
    return true;
}

} // namespace ortho_residency
} // namespace opencalibration_amd
