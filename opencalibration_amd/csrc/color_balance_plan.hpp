// Colour balance: the plan of one solve - how the correspondences are grouped into chunks, in which order the unknowns
// stand, which block envelope that gives, and which chunk records every entry of the normal equations sums - and the
// pieces of arithmetic the device kernels (color_balance.hip) are made of, written so that the host can run them too:
// plan_evaluate_host() below forms cost, J'J and J'r from the same functions in the same order as the kernels, so what
// the device computes is defined here and the tests hold the device to it bit for bit.
#pragma once

#include "color_balance.hpp"
#include "../../include/ochip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

namespace ochip_cb
{

constexpr int NB = 64;         // the system's tile size (relax_lm.hpp: LM_NB)
constexpr int CHUNK = 64;      // correspondences per record
constexpr int REC = 192;       // doubles per record: BLOCK_TRI (171) + 18 + 1, padded
constexpr int REC_ENTRIES = BLOCK_TRI + BLOCK_COLS + 1;
constexpr int REC_G = BLOCK_TRI, REC_COST = BLOCK_TRI + BLOCK_COLS;
constexpr int JROW = 3 * BLOCK_COLS + 3; // a correspondence's row of a chunk's work area: J, residuals (odd: no LDS bank conflicts over k)
constexpr int FINISH_WIDTH = 256;        // partial sums of the finishing kernel (relax_lm.hpp: LM_TG)
constexpr int SEGMENT = 256;             // an owner with more records than this is summed in two levels
constexpr int GATHER_SLICES = 4;         // interleaved partial sums of an owner's records

struct cb_obs
{
    obs o;
    uint32_t flip, pad;
};
static_assert(sizeof(cb_obs) == 64, "cb_obs layout");

struct cb_chunk
{
    uint32_t first, count;          // its correspondences (grouped order)
    int32_t t_lo, t_hi, t_vlo, t_vhi; // first unknown of the pair's cameras and of their models
    uint32_t shared, pad;
};

enum
{
    OWN_CAM = 0,        // a camera's 6 x 6 diagonal block and gradient; item code bit 0: the camera is the chunk's second
    OWN_PAIR = 1,       // the 6 x 6 block of a camera pair; swap: the row camera is the chunks' first
    OWN_CAM_MODEL = 2,  // model rows x camera columns (3 x 6); code bit 0: camera side, bit 1: vignetting side
    OWN_MODEL = 3,      // a model's 3 x 3 diagonal block and gradient; code bit 1: vignetting side
    OWN_MODEL_PAIR = 4, // 3 x 3 block of two models; code bit 0: the row model is the chunk's first side
};
struct cb_owner
{
    uint32_t first, count; // items
    int32_t type, row, col, swap;
    uint32_t seg_first, seg_count; // count > SEGMENT: its items are summed by segments first (seg_count > 0)
};

// correspondence k of a chunk at the state x: corrected residuals, Jacobian (J != nullptr) and cost
OCHIP_CB_HD bool chunk_eval(const cb_obs *obs, const cb_chunk &c, uint32_t k, const double *x, double *res, double *J, double *cost)
{
    const cb_obs ob = obs[c.first + k];
    const bool flip = ob.flip != 0, shared = c.shared != 0;
    const double *const cam[2] = {x + (flip ? c.t_hi : c.t_lo), x + (flip ? c.t_lo : c.t_hi)};
    const double *const vig[2] = {x + (shared || !flip ? c.t_vlo : c.t_vhi), x + (shared ? c.t_vlo : (flip ? c.t_vlo : c.t_vhi))};
    return eval_block(ob.o, cam, vig, shared, flip, res, J, cost);
}

// entry e of a chunk's record from the chunk's work area (rows: count x JROW, costs: count): the packed lower triangle
// of J'J, then J'r, then the cost, each summed over the correspondences in index order
OCHIP_CB_HD double record_entry(const double *rows, const double *costs, uint32_t count, int e)
{
    double s = 0;
    if (e < REC_G)
    {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e)
            i++;
        const int j = e - i * (i + 1) / 2;
        for (uint32_t k = 0; k < count; k++)
            s += jtj_entry(rows + k * JROW, i, j);
    }
    else if (e < REC_COST)
        for (uint32_t k = 0; k < count; k++)
            s += jtr_entry(rows + k * JROW, rows + k * JROW + 3 * BLOCK_COLS, e - REC_G);
    else
        for (uint32_t k = 0; k < count; k++)
            s += costs[k];
    return s;
}

// where entry e of an owner's block lies in a record (packed lower triangle of the 18 local columns, then the gradient)
OCHIP_CB_HD int owner_entry(int type, int swap, int e, int code, int *di, int *dj, bool *is_g)
{
    *is_g = false;
    const int cs = code & 1, vs = (code >> 1) & 1;
    if (type == OWN_CAM || type == OWN_MODEL)
    {
        const int tri = type == OWN_CAM ? 21 : 6, base = type == OWN_CAM ? 6 * cs : 12 + 3 * vs;
        if (e >= tri)
        {
            *is_g = true;
            *di = e - tri;
            return REC_G + base + e - tri;
        }
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e)
            i++;
        const int j = e - i * (i + 1) / 2;
        *di = i, *dj = j;
        return tri_index(base + i, base + j);
    }
    if (type == OWN_PAIR)
    {
        const int i = e / 6, j = e % 6;
        *di = i, *dj = j;
        return swap ? tri_index(6 + j, i) : tri_index(6 + i, j);
    }
    if (type == OWN_CAM_MODEL)
    {
        const int i = e / 6, j = e % 6;
        *di = i, *dj = j;
        return tri_index(12 + 3 * vs + i, 6 * cs + j);
    }
    const int i = e / 3, j = e % 3; // OWN_MODEL_PAIR
    *di = i, *dj = j;
    return cs ? tri_index(15 + j, 12 + i) : tri_index(15 + i, 12 + j);
}

OCHIP_CB_HD int owner_entries(int type)
{
    return type == OWN_CAM ? 27 : type == OWN_PAIR ? 36 : type == OWN_CAM_MODEL ? 18 : 9;
}

// slice `slice` of entry e over the records items[first .. first + count): records slice, slice + GATHER_SLICES, ... in order
OCHIP_CB_HD double items_slice(const double *rec, const uint32_t *items, int type, int swap, uint32_t first, uint32_t count, int e,
                               int slice)
{
    int di = 0, dj = 0;
    bool is_g = false;
    double s = 0;
    for (uint32_t k = (uint32_t)slice; k < count; k += GATHER_SLICES)
    {
        const uint32_t it = items[first + k];
        s += rec[(size_t)(it >> 3) * REC + owner_entry(type, swap, e, (int)(it & 7), &di, &dj, &is_g)];
    }
    return s;
}

// One segment of a large owner (SEGMENT records; with a single camera model every chunk is a record of that model's
// block, and one workgroup walking them all would be the longest chain of an evaluation): entry e of its partial sum
struct cb_segment
{
    uint32_t first, count; // items
    int32_t type, swap;
};
OCHIP_CB_HD double fold_slices(const double *part /* [GATHER_SLICES] */)
{
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// slice `slice` of entry e of an owner: over its records, or over its segments' partial sums (partial: [segment][64])
OCHIP_CB_HD double gather_slice(const double *rec, const uint32_t *items, const double *partial, const cb_owner &o, int e, int slice)
{
    if (o.seg_count == 0)
        return items_slice(rec, items, o.type, o.swap, o.first, o.count, e, slice);
    double s = 0;
    for (uint32_t k = (uint32_t)slice; k < o.seg_count; k += GATHER_SLICES)
        s += partial[(size_t)(o.seg_first + k) * 64 + e];
    return s;
}

// entry e of an owner from its slices, priors added: the value, and where it goes - *is_g: g[*row], else A(*row, *col)
OCHIP_CB_HD double gather_value(const double *part /* [GATHER_SLICES] */, const cb_owner &o, int e, const double *weight, const double *x,
                                int *row, int *col, bool *is_g)
{
    int di = 0, dj = 0;
    owner_entry(o.type, o.swap, e, 0, &di, &dj, is_g);
    double v = fold_slices(part);
    *row = o.row + di, *col = o.col + dj;
    if (*is_g)
    {
        const double w = weight[o.row + di];
        return v + w * (w * x[o.row + di]);
    }
    if ((o.type == OWN_CAM || o.type == OWN_MODEL) && di == dj)
    {
        const double w = weight[o.row + di];
        v += w * w;
    }
    return v;
}

// the sum of v[0 .. n) the finishing kernel forms: `width` strided partial sums, then a binary tree over them
OCHIP_CB_HD double tree_fold(double *sh, int width) // sh[0 .. width) -> the total (sh is overwritten)
{
    for (int s = width / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; t++)
            sh[t] += sh[t + s];
    return sh[0];
}

// ---- the plan (host) ---------------------------------------------------------------------------------------------------
struct plan
{
    uint32_t n_cams = 0, n_models = 0;
    uint64_t n_corr = 0;
    int n = 0; // unknowns
    std::vector<int32_t> cam_t, model_t; // first unknown of every camera / model (table order)
    std::vector<cb_obs> obs;             // grouped order
    std::vector<cb_chunk> chunks;
    std::vector<cb_owner> owners;
    std::vector<uint32_t> items; // chunk << 3 | code
    std::vector<cb_segment> segments; // of the owners with more than SEGMENT records
    std::vector<double> weight;  // per unknown: the prior's weight
    // the block envelope (relax_lm.hpp: lm_envelope)
    std::vector<int> env_end, first_col, region_begin;
    int tail_begin = 0, n_separators = 0;
};

inline bool plan_fail(std::string *err, const char *fmt, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
    return false;
}

// Order of the cameras' unknowns: reverse Cuthill-McKee over the pair graph, then the dissection into regions
// (relax.hip, assign_tangent, with 6 unknowns per camera: a region of g cameras, g a multiple of 32, is 3 g / 32
// tiles).  order: camera rows in the order of their unknowns, the last *n_separators of them the separators;
// region_first_block: lm_envelope::region_begin.
inline void order_cameras(uint32_t n_cams, const std::vector<std::pair<uint32_t, uint32_t>> &pairs, std::vector<uint32_t> *order_out,
                   int *n_separators, std::vector<int> *region_first_block)
{
    std::vector<uint32_t> order(n_cams);
    std::iota(order.begin(), order.end(), 0u);
    *n_separators = 0;
    region_first_block->clear();
    constexpr int PER_TILE_CAMS = 32; // 32 cameras = 192 unknowns = 3 tiles
    if (n_cams > (uint32_t)NB / 3)
    {
        std::vector<std::vector<uint32_t>> adj(n_cams);
        for (const auto &p : pairs)
        {
            adj[p.first].push_back(p.second);
            adj[p.second].push_back(p.first);
        }
        for (auto &l : adj)
            std::sort(l.begin(), l.end(), [&](uint32_t x, uint32_t y) {
                return adj[x].size() != adj[y].size() ? adj[x].size() < adj[y].size() : x < y;
            });
        std::vector<char> seen(n_cams, 0);
        order.clear();
        auto bfs = [&](uint32_t start, std::vector<uint32_t> &out, std::vector<char> &mark) {
            const size_t first = out.size();
            out.push_back(start);
            mark[start] = 1;
            for (size_t h = first; h < out.size(); h++)
                for (uint32_t v : adj[out[h]])
                    if (!mark[v])
                    {
                        mark[v] = 1;
                        out.push_back(v);
                    }
        };
        for (uint32_t s0 = 0; s0 < n_cams; s0++)
        {
            if (seen[s0])
                continue;
            // the component of s0, its lowest-degree member, then two sweeps towards the periphery
            std::vector<uint32_t> comp;
            std::vector<char> tmp(seen);
            bfs(s0, comp, tmp);
            uint32_t start = comp[0];
            for (uint32_t v : comp)
                if (adj[v].size() < adj[start].size() || (adj[v].size() == adj[start].size() && v < start))
                    start = v;
            for (int sweep = 0; sweep < 2; sweep++)
            {
                std::vector<uint32_t> lv;
                std::vector<char> tmp2(seen);
                bfs(start, lv, tmp2);
                start = lv.back();
            }
            bfs(start, order, seen);
        }
        std::reverse(order.begin(), order.end());
        const int N = (int)n_cams;
        if (N >= 2 * NB)
        {
            auto cut = [&](int g, std::vector<int> *state_out, int *n_regions) -> int { // -> path length in cameras (or -1)
                std::vector<int> state((size_t)N, -1);                                  // by camera: region, or -2 = separator
                int left = N, regions = 0, longest = 0, seps = 0;
                size_t pos = 0;
                while (left > 0)
                {
                    const bool last = left <= g + g / 2;
                    const int want = last ? left : g;
                    int got = 0;
                    std::vector<uint32_t> mine;
                    for (; pos < order.size() && got < want; pos++)
                        if (state[order[pos]] == -1)
                        {
                            state[order[pos]] = regions;
                            mine.push_back(order[pos]);
                            got++;
                        }
                    left -= got;
                    longest = std::max(longest, got);
                    regions++;
                    if (last)
                        break;
                    for (uint32_t v : mine)
                        for (uint32_t u : adj[v])
                            if (state[u] == -1)
                            {
                                state[u] = -2;
                                seps++;
                                left--;
                            }
                }
                if (regions < 2)
                    return -1;
                if (state_out)
                    state_out->swap(state);
                *n_regions = regions;
                return longest + seps + seps / 2; // (a column of the tail costs more than a column of a region)
            };
            int best_g = 0, best_path = N, regions = 0;
            for (int g = PER_TILE_CAMS; g <= N / 2; g += PER_TILE_CAMS)
            {
                int r = 0;
                const int path = cut(g, nullptr, &r);
                if (path >= 0 && path < best_path)
                    best_path = path, best_g = g;
            }
            if (best_g > 0 && 10 * best_path <= 8 * N)
            {
                std::vector<int> state;
                cut(best_g, &state, &regions);
                std::vector<uint32_t> cut_order;
                for (uint32_t v : order)
                    if (state[v] >= 0)
                        cut_order.push_back(v);
                for (uint32_t v : order)
                    if (state[v] == -2)
                    {
                        cut_order.push_back(v);
                        (*n_separators)++;
                    }
                std::stable_sort(cut_order.begin(), cut_order.end() - *n_separators,
                                 [&](uint32_t a, uint32_t b) { return state[a] < state[b]; });
                order.swap(cut_order);
                for (int r = 0; r < regions; r++)
                    region_first_block->push_back(r * (CAM_UNKNOWNS * best_g / NB));
            }
        }
    }
    order_out->swap(order);
}

// cam_ids, model_ids: sorted, unique, holding every id the correspondences name
inline bool build_plan(const ochip_color_corr *corr, uint64_t n_corr, const uint64_t *cam_ids, uint32_t n_cams, const uint32_t *model_ids,
                       uint32_t n_models, plan *p, std::string *err)
{
    if (!corr || !n_corr || !cam_ids || !n_cams || !model_ids || !n_models)
        return plan_fail(err, "colour balance: no correspondences or no id tables");
    if (n_corr >= (1ull << 29) || (uint64_t)n_cams * CAM_UNKNOWNS + (uint64_t)n_models * MODEL_UNKNOWNS > (1u << 24))
        return plan_fail(err, "colour balance: problem too large");
    for (uint32_t i = 1; i < n_cams; i++)
        if (!(cam_ids[i - 1] < cam_ids[i]))
            return plan_fail(err, "colour balance: camera ids must be sorted and unique");
    for (uint32_t i = 1; i < n_models; i++)
        if (!(model_ids[i - 1] < model_ids[i]))
            return plan_fail(err, "colour balance: model ids must be sorted and unique");
    p->n_cams = n_cams, p->n_models = n_models, p->n_corr = n_corr;
    // ---- table rows, counts, the group of every correspondence
    struct keyed
    {
        uint32_t lo, hi, mlo, mhi, flip;
        uint64_t index;
    };
    std::vector<keyed> ks(n_corr);
    std::vector<uint64_t> cam_count(n_cams, 0), model_count(n_models, 0);
    for (uint64_t i = 0; i < n_corr; i++)
    {
        const ochip_color_corr &c = corr[i];
        const uint32_t a = (uint32_t)(std::lower_bound(cam_ids, cam_ids + n_cams, c.camera_id_a) - cam_ids);
        const uint32_t b = (uint32_t)(std::lower_bound(cam_ids, cam_ids + n_cams, c.camera_id_b) - cam_ids);
        const uint32_t ma = (uint32_t)(std::lower_bound(model_ids, model_ids + n_models, c.model_id_a) - model_ids);
        const uint32_t mb = (uint32_t)(std::lower_bound(model_ids, model_ids + n_models, c.model_id_b) - model_ids);
        if (a >= n_cams || cam_ids[a] != c.camera_id_a || b >= n_cams || cam_ids[b] != c.camera_id_b || ma >= n_models ||
            model_ids[ma] != c.model_id_a || mb >= n_models || model_ids[mb] != c.model_id_b)
            return plan_fail(err, "colour balance: correspondence %llu names an id that is not in the tables",
                              (unsigned long long)i);
        if (a == b)
            return plan_fail(err, "colour balance: correspondence %llu pairs camera %llu with itself",
                              (unsigned long long)i, (unsigned long long)c.camera_id_a);
        cam_count[a]++, cam_count[b]++, model_count[ma]++, model_count[mb]++;
        const bool flip = a > b;
        ks[i] = keyed{flip ? b : a, flip ? a : b, flip ? mb : ma, flip ? ma : mb, flip ? 1u : 0u, i};
    }
    std::stable_sort(ks.begin(), ks.end(), [](const keyed &x, const keyed &y) {
        if (x.lo != y.lo)
            return x.lo < y.lo;
        if (x.hi != y.hi)
            return x.hi < y.hi;
        if (x.mlo != y.mlo)
            return x.mlo < y.mlo;
        return x.mhi < y.mhi;
    });
    // ---- the order of the unknowns and the envelope
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (uint64_t i = 0; i < n_corr; i++)
        if (i == 0 || ks[i].lo != ks[i - 1].lo || ks[i].hi != ks[i - 1].hi)
            pairs.emplace_back(ks[i].lo, ks[i].hi);
    std::vector<uint32_t> order;
    std::vector<int> region_first_block;
    int n_separators = 0;
    order_cameras(n_cams, pairs, &order, &n_separators, &region_first_block);
    p->cam_t.assign(n_cams, -1);
    int t = 0;
    for (uint32_t c : order)
    {
        p->cam_t[c] = t;
        t += CAM_UNKNOWNS;
    }
    p->model_t.assign(n_models, -1);
    for (uint32_t m = 0; m < n_models; m++)
    {
        p->model_t[m] = t;
        t += MODEL_UNKNOWNS;
    }
    const int n = t;
    struct
    {
        std::vector<int> env_end, first_col, region_begin;
        int tail_begin = 0;
    } env;
    {
        const int cam_end = CAM_UNKNOWNS * ((int)n_cams - n_separators), nblk = (n + NB - 1) / NB;
        env.tail_begin = cam_end;
        env.region_begin = region_first_block;
        env.env_end.assign(nblk, 0);
        for (int k = 0; k < nblk; k++)
            env.env_end[k] = std::min((k + 1) * NB, cam_end);
        for (uint32_t c = 0; c < n_cams; c++) // a camera's own block may straddle two column blocks
            if (p->cam_t[c] < cam_end)
                for (int k = p->cam_t[c] / NB; k <= (p->cam_t[c] + CAM_UNKNOWNS - 1) / NB; k++)
                    env.env_end[k] = std::max(env.env_end[k], p->cam_t[c] + CAM_UNKNOWNS);
        for (const auto &pr : pairs)
        {
            const int ta = p->cam_t[pr.first], tb = p->cam_t[pr.second];
            if (std::max(ta, tb) >= cam_end)
                continue;
            const int lo = std::min(ta, tb), hi = std::max(ta, tb) + CAM_UNKNOWNS;
            for (int k = lo / NB; k <= (lo + CAM_UNKNOWNS - 1) / NB; k++)
                env.env_end[k] = std::max(env.env_end[k], hi);
        }
        for (int k = 1; k < nblk; k++)
            env.env_end[k] = std::max(env.env_end[k], std::min(env.env_end[k - 1], cam_end));
        env.first_col.assign(nblk, 0);
        for (int k = 0; k < nblk; k++)
        {
            const int k0 = k * NB;
            int first = k0;
            if (k0 + NB > cam_end) // the block holds tail rows: dense
                first = 0;
            else
                for (int c = 0; c < k; c++)
                    if (env.env_end[c] > k0)
                    {
                        first = c * NB;
                        break;
                    }
            env.first_col[k] = first;
        }
    }
    // ---- chunks, observations in grouped order, owners and their items
    std::vector<cb_obs> obs(n_corr);
    std::vector<cb_chunk> chunks;
    for (uint64_t i = 0; i < n_corr; i++)
    {
        const ochip_color_corr &c = corr[ks[i].index];
        cb_obs &o = obs[i];
        for (int k = 0; k < 3; k++)
            o.o.lab[0][k] = c.lab_a[k], o.o.lab[1][k] = c.lab_b[k];
        o.o.radius[0] = c.normalized_radius_a, o.o.radius[1] = c.normalized_radius_b;
        o.o.angle[0] = c.view_angle_a, o.o.angle[1] = c.view_angle_b;
        o.o.nx[0] = c.normalized_x_a, o.o.nx[1] = c.normalized_x_b;
        o.o.ny[0] = c.normalized_y_a, o.o.ny[1] = c.normalized_y_b;
        o.flip = ks[i].flip, o.pad = 0;
        const bool new_group = i == 0 || ks[i].lo != ks[i - 1].lo || ks[i].hi != ks[i - 1].hi || ks[i].mlo != ks[i - 1].mlo ||
                               ks[i].mhi != ks[i - 1].mhi;
        if (new_group || chunks.back().count == CHUNK)
            chunks.push_back(cb_chunk{(uint32_t)i, 0, p->cam_t[ks[i].lo], p->cam_t[ks[i].hi], p->model_t[ks[i].mlo],
                                      p->model_t[ks[i].mhi], ks[i].mlo == ks[i].mhi ? 1u : 0u, 0});
        chunks.back().count++;
    }
    // an owner is named by (type, row unknown, column unknown); its items by (chunk, code), in chunk order
    struct item
    {
        int32_t type, row, col, swap;
        uint32_t packed;
    };
    std::vector<item> its;
    its.reserve(chunks.size() * 12);
    for (uint32_t k = 0; k < (uint32_t)chunks.size(); k++)
    {
        const cb_chunk &c = chunks[k];
        auto add = [&](int type, int row, int col, int swap, uint32_t code) { its.push_back(item{type, row, col, swap, k << 3 | code}); };
        add(OWN_CAM, c.t_lo, c.t_lo, 0, 0);
        add(OWN_CAM, c.t_hi, c.t_hi, 0, 1);
        const bool swap = c.t_hi < c.t_lo;
        add(OWN_PAIR, swap ? c.t_lo : c.t_hi, swap ? c.t_hi : c.t_lo, swap ? 1 : 0, 0);
        for (uint32_t cs = 0; cs < 2; cs++)
            for (uint32_t vs = 0; vs < (c.shared ? 1u : 2u); vs++)
                add(OWN_CAM_MODEL, vs ? c.t_vhi : c.t_vlo, cs ? c.t_hi : c.t_lo, 0, cs | vs << 1);
        add(OWN_MODEL, c.t_vlo, c.t_vlo, 0, 0);
        if (!c.shared)
        {
            add(OWN_MODEL, c.t_vhi, c.t_vhi, 0, 2);
            const bool row_is_lo = c.t_vlo > c.t_vhi;
            add(OWN_MODEL_PAIR, row_is_lo ? c.t_vlo : c.t_vhi, row_is_lo ? c.t_vhi : c.t_vlo, 0, row_is_lo ? 1 : 0);
        }
    }
    std::stable_sort(its.begin(), its.end(), [](const item &a, const item &b) {
        if (a.type != b.type)
            return a.type < b.type;
        if (a.row != b.row)
            return a.row < b.row;
        return a.col < b.col;
    });
    std::vector<cb_owner> owners;
    std::vector<uint32_t> items(its.size());
    for (size_t i = 0; i < its.size(); i++)
    {
        items[i] = its[i].packed;
        if (i == 0 || its[i].type != its[i - 1].type || its[i].row != its[i - 1].row || its[i].col != its[i - 1].col)
            owners.push_back(cb_owner{(uint32_t)i, 0, its[i].type, its[i].row, its[i].col, its[i].swap, 0, 0});
        owners.back().count++;
    }
    std::vector<double> weight(n);
    for (uint32_t c = 0; c < n_cams; c++)
        for (int k = 0; k < CAM_UNKNOWNS; k++)
            weight[p->cam_t[c] + k] = prior_weight(cam_count[c]);
    for (uint32_t m = 0; m < n_models; m++)
        for (int k = 0; k < MODEL_UNKNOWNS; k++)
            weight[p->model_t[m] + k] = prior_weight(model_count[m]);
    p->n = n;
    p->n_separators = n_separators;
    p->env_end = env.env_end, p->first_col = env.first_col, p->region_begin = env.region_begin, p->tail_begin = env.tail_begin;
    for (cb_owner &o : owners)
        if (o.count > (uint32_t)SEGMENT)
        {
            o.seg_first = (uint32_t)p->segments.size();
            for (uint32_t f = 0; f < o.count; f += SEGMENT)
                p->segments.push_back(cb_segment{o.first + f, std::min<uint32_t>(SEGMENT, o.count - f), o.type, o.swap});
            o.seg_count = (uint32_t)p->segments.size() - o.seg_first;
        }
    p->obs.swap(obs), p->chunks.swap(chunks), p->owners.swap(owners), p->items.swap(items), p->weight.swap(weight);
    return true;
}

// What the device's evaluation computes, on the host: the same functions in the same order.  x: the state in the plan's
// unknown order.  JtJ (n x n, both triangles) and Jtr may be nullptr (the cost-only evaluation).  false: a residual is
// not finite.
inline bool plan_evaluate_host(const plan &P, const double *x, double *cost, double *JtJ, double *Jtr)
{
    const size_t nch = P.chunks.size(), n = (size_t)P.n;
    std::vector<double> rec(JtJ ? nch * REC : 0), chunk_cost(nch), rows((size_t)CHUNK * JROW), costs(CHUNK);
    bool finite = true;
    for (size_t c = 0; c < nch; c++)
    {
        const cb_chunk &ch = P.chunks[c];
        for (uint32_t k = 0; k < ch.count; k++)
        {
            double res[3];
            double *r = rows.data() + (size_t)k * JROW;
            finite = chunk_eval(P.obs.data(), ch, k, x, res, JtJ ? r : nullptr, &costs[k]) && finite;
            r[3 * BLOCK_COLS] = res[0], r[3 * BLOCK_COLS + 1] = res[1], r[3 * BLOCK_COLS + 2] = res[2];
        }
        chunk_cost[c] = record_entry(rows.data(), costs.data(), ch.count, REC_COST);
        if (JtJ)
            for (int e = 0; e < REC_ENTRIES; e++)
                rec[c * REC + e] = e == REC_COST ? chunk_cost[c] : record_entry(rows.data(), costs.data(), ch.count, e);
    }
    if (JtJ)
    {
        std::fill(JtJ, JtJ + n * n, 0.0);
        std::fill(Jtr, Jtr + n, 0.0);
        std::vector<double> partial(P.segments.size() * 64, 0.0);
        for (size_t g = 0; g < P.segments.size(); g++)
            for (int e = 0; e < owner_entries(P.segments[g].type); e++)
            {
                const cb_segment &sg = P.segments[g];
                double part[GATHER_SLICES];
                for (int s = 0; s < GATHER_SLICES; s++)
                    part[s] = items_slice(rec.data(), P.items.data(), sg.type, sg.swap, sg.first, sg.count, e, s);
                partial[g * 64 + e] = fold_slices(part);
            }
        for (const cb_owner &o : P.owners)
            for (int e = 0; e < owner_entries(o.type); e++)
            {
                double part[GATHER_SLICES];
                for (int s = 0; s < GATHER_SLICES; s++)
                    part[s] = gather_slice(rec.data(), P.items.data(), partial.data(), o, e, s);
                int row = 0, col = 0;
                bool is_g = false;
                const double v = gather_value(part, o, e, P.weight.data(), x, &row, &col, &is_g);
                if (is_g)
                    Jtr[row] = v;
                else
                    JtJ[(size_t)row * n + col] = JtJ[(size_t)col * n + row] = v;
            }
    }
    // the finishing kernel's sums: 256 strided partial sums each, folded by a binary tree
    constexpr int TG = FINISH_WIDTH;
    double a[TG], b[TG];
    for (int t = 0; t < TG; t++)
    {
        a[t] = b[t] = 0;
        for (size_t k = (size_t)t; k < nch; k += TG)
            a[t] += chunk_cost[k];
        for (size_t i = (size_t)t; i < n; i += TG)
        {
            const double r = P.weight[i] * x[i];
            b[t] += 0.5 * (r * r);
        }
    }
    const double matches = tree_fold(a, TG), priors = tree_fold(b, TG);
    *cost = matches + priors;
    return finite;
}

} // namespace ochip_cb
