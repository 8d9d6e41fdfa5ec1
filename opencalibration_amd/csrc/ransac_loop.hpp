// The parts of ransac<Model> (src/model_inliers/ransac.cpp:53-257) that do not depend on the model, one wavefront per pair
// (gfx950): the sample stream, PROSAC's pool and sample, the MSAC / SPRT scoring walk, the adaptive iteration count, the
// per-pair scratch and the exits without a model.  The reference has one loop for its three models; here the homography
// loop (ransac.hip) and the fundamental- / essential-matrix loop (ransac_epipolar.hip) stay two functions - they differ in
// what surrounds these parts - and call them in the reference's order.
//
// libstdc++ pieces on the result path: std::default_random_engine (= minstd_rand0) and
// std::uniform_int_distribution<size_t> are re-implemented here exactly (bits/random.tcc,
// bits/uniform_int_dist.h "downscaling" branch); std::sort (PROSAC order) and std::shuffle
// (evaluation order) are executed on the host with the real libstdc++ and handed in.
#pragma once

#include "ctx.hpp"

#include <cmath>

namespace
{

constexpr int W = 64;
// -DOCHIP_RANSAC_PHASES: shader-clock cycles per phase of ransac_homography_kernel, summed over the wavefronts of a launch and
// printed by the host after it (how the kernel's time divides; not part of the product build)
#ifdef OCHIP_RANSAC_PHASES
static __device__ unsigned long long g_phase[16];
#define OCHIP_PHASE_T0(t) const unsigned long long t = clock64()
#define OCHIP_PHASE_ADD(t, slot)                                                                                       \
    do                                                                                                                 \
    {                                                                                                                  \
        if (threadIdx.x == 0)                                                                                          \
            atomicAdd(&g_phase[slot], clock64() - t);                                                                  \
    } while (0)
#define OCHIP_PHASE_COUNT(slot, n)                                                                                     \
    do                                                                                                                 \
    {                                                                                                                  \
        if (threadIdx.x == 0)                                                                                          \
            atomicAdd(&g_phase[slot], (unsigned long long)(n));                                                        \
    } while (0)
#else
#define OCHIP_PHASE_T0(t)
#define OCHIP_PHASE_ADD(t, slot)
#define OCHIP_PHASE_COUNT(slot, n)
#endif
constexpr uint32_t MIN_ITERATIONS = 20, MAX_ITERATIONS = 10000, MAX_INNER_ITERATIONS = 5;

__device__ __forceinline__ double bcast(double v, int src_lane)
{
    union {
        double d;
        uint32_t u[2];
    } x;
    x.d = v;
    x.u[0] = __builtin_amdgcn_readlane(x.u[0], src_lane);
    x.u[1] = __builtin_amdgcn_readlane(x.u[1], src_lane);
    return x.d;
}

__device__ __forceinline__ uint32_t minstd_next(uint32_t &x) // std::minstd_rand0: x = 16807 x mod (2^31 - 1)
{
    x = (uint32_t)(((uint64_t)x * 16807ull) % 2147483647ull);
    return x;
}

// std::uniform_int_distribution<size_t>(0, hi)(minstd_rand0) — bits/uniform_int_dist.h, urngrange > urange.
// urngrange = max() - min() = 2147483646 - 1 and every operand stays below 2^31, so 32-bit arithmetic gives the
// 64-bit results; the scaling only depends on hi and is shared by the draws of one sample.
struct uniform_range
{
    uint32_t scaling, past;
};
__device__ __forceinline__ uniform_range make_range(uint32_t hi)
{
    const uint32_t uerange = hi + 1;
    uniform_range r;
    r.scaling = 2147483645u / uerange;
    r.past = uerange * r.scaling;
    return r;
}
__device__ __forceinline__ uint32_t uniform_int(uint32_t &x, const uniform_range &r)
{
    uint32_t ret;
    do
        ret = minstd_next(x) - 1u;
    while (ret >= r.past);
    return ret / r.scaling;
}

struct pair_data // per-pair scratch in HBM (L2 resident while the pair is being processed)
{
    double *x1, *y1, *x2, *y2;     // [M] normalised coordinates, correspondence order (the kernel's prologue fills them)
    double *ex1, *ey1, *ex2, *ey2; // [M] the same in shuffled evaluation order (position p holds eval_order[p])
    uint8_t *cand, *inl;           // [M] candidate / current inlier flags, indexed by correspondence
    double *P;                     // column-major (2M+1) x 9 system of fitInliers
    uint32_t M;
};

// The pair's share of the launch's scratch, bound in two steps around the kernel's prologue.  Before it: the 8 coordinate
// planes of `total` doubles each, which the prologue fills.
__device__ __forceinline__ pair_data bind_coords(double *coord_scratch, uint64_t total, uint64_t offset, uint32_t M)
{
    pair_data pd;
    pd.x1 = coord_scratch + offset;
    pd.y1 = coord_scratch + total + offset;
    pd.x2 = coord_scratch + 2 * total + offset;
    pd.y2 = coord_scratch + 3 * total + offset;
    pd.ex1 = coord_scratch + 4 * total + offset;
    pd.ey1 = coord_scratch + 5 * total + offset;
    pd.ex2 = coord_scratch + 6 * total + offset;
    pd.ey2 = coord_scratch + 7 * total + offset;
    pd.cand = pd.inl = nullptr;
    pd.P = nullptr;
    pd.M = M;
    return pd;
}
// After it: the flag planes of `total` bytes - two that trade places on every improvement (the candidates of the improving
// model become the inliers; a model that needs more takes the planes behind them) - and the job's 81 doubles.  SEARCH ==
// false (a refit samples nothing): no flags of a hypothesis, `inl` is the caller's.
template <bool SEARCH>
__device__ __forceinline__ void bind_scratch(pair_data &pd, uint8_t *flag_scratch, double *P_scratch, uint64_t total, uint64_t offset,
                                             uint32_t job_id)
{
    if (SEARCH)
    {
        pd.cand = flag_scratch + offset;
        pd.inl = flag_scratch + total + offset;
    }
    pd.P = P_scratch + 81 * (size_t)job_id;
}

// What a pair without a model returns, and the exit of a pair with fewer matches than a sample (ransac.cpp:67-70)
__device__ __forceinline__ ochip_ransac_result empty_result()
{
    ochip_ransac_result res;
    for (int i = 0; i < 9; i++)
        res.H[i] = __builtin_nan("");
    res.score = 0;
    res.iterations = 0;
    res.n_inliers = 0;
    res.improvements = 0;
    res.reserved = 0;
    return res;
}
__device__ __forceinline__ void too_few_matches(const ochip_ransac_result &res, uint32_t M, uint8_t *inliers, ochip_ransac_result *result)
{
    for (uint32_t i = threadIdx.x; i < M; i += W)
        inliers[i] = 0;
    if (threadIdx.x == 0)
        *result = res;
}

// positions first .. K - 1 of a sample: distinct positions of the sampling pool [0, hi]; distinct positions are distinct
// correspondences because the PROSAC order is a permutation, so the uniqueness test of ransac.cpp:115-122 / :142-149 needs no loaded
// value and the sorted_idx reads of a sample go out together
template <int K> __device__ __forceinline__ void draw_distinct(uint32_t &rng, uint32_t hi, int first, uint32_t *c)
{
    const uniform_range range = make_range(hi);
    for (int j = first; j < K; j++)
    {
        uint32_t cand;
        bool unique;
        do
        {
            cand = uniform_int(rng, range);
            unique = true;
            for (int k = first; k < j; k++)
                if (c[k] == cand)
                    unique = false;
        } while (!unique);
        c[j] = cand;
    }
}

// PROSAC (the matches have qualities): the pool grows by one every tenth iteration (ransac.cpp:164-165)
__device__ __forceinline__ void prosac_grow(uint32_t it, uint32_t &prosac_n, uint32_t M)
{
    if (prosac_n < M && it > 0 && it % 10 == 0)
        prosac_n++;
}

// the minimal sample (ransac.cpp:104-154, :167-171): K correspondences (MAPPED: positions of the pool taken through the PROSAC
// order sorted_idx when the matches have qualities), or the K positions themselves (the fast-forward's replay, which only
// loads the correspondences of the lane that keeps the sample).  A pool that has grown takes its newest member and draws
// the rest from the ones before it.
template <int K, bool MAPPED>
__device__ __forceinline__ void draw_sample(uint32_t &rng, uint32_t prosac_n, uint32_t M, bool has_quality, const uint32_t *sorted_idx,
                                            uint32_t *s)
{
    uint32_t c[K];
    if (has_quality && prosac_n < M && prosac_n > (uint32_t)K)
    {
        c[0] = prosac_n - 1; // never drawn again: the others come from [0, prosac_n - 2]
        draw_distinct<K>(rng, prosac_n - 2, 1, c);
        for (int j = 0; j < K; j++)
            s[j] = MAPPED ? sorted_idx[c[j]] : c[j];
    }
    else
    {
        draw_distinct<K>(rng, (has_quality ? prosac_n : M) - 1, 0, c);
        for (int j = 0; j < K; j++)
            s[j] = MAPPED && has_quality ? sorted_idx[c[j]] : c[j];
    }
}

// MSAC scoring of one model; its error is model_error(m, x1, y1, x2, y2), an overload per model.  ORDERED: walk the shuffled
// eval_order and apply the SPRT early exit of ransac.cpp:181-205; otherwise natural order, no exit (Model::evaluate).
// The running sum is accumulated one element at a time in walk order (non-inliers add +0.0, which changes nothing,
// so the chain is a fixed 64 adds per chunk with the addend taken from lane l by v_readlane).  The walk is
// software-pipelined: the next chunk's coordinates are requested before this chunk's arithmetic, and the ORDERED walk
// reads coordinates that the prologue stored in evaluation order, so every load of the 20+ scorings of a pair is a
// coalesced stream (the gather through eval_order cost two dependent memory round trips per 64 matches).
template <bool ORDERED, class Model>
__device__ double score_walk(const Model &m, const pair_data &pd, const uint32_t *__restrict__ order, uint8_t *flags,
                             double thr, double best_score, bool *rejected, uint32_t *n_inliers)
{
    const int lane = threadIdx.x;
    const uint32_t M = pd.M;
    const double *X1 = ORDERED ? pd.ex1 : pd.x1, *Y1 = ORDERED ? pd.ey1 : pd.y1, *X2 = ORDERED ? pd.ex2 : pd.x2,
                 *Y2 = ORDERED ? pd.ey2 : pd.y2;
    double s = 0;
    uint32_t count = 0;
    *rejected = false;
    double nx1, ny1, nx2, ny2;
    uint32_t nidx;
    {
        const bool nv = (uint32_t)lane < M;
        nx1 = nv ? X1[lane] : 0.0, ny1 = nv ? Y1[lane] : 0.0, nx2 = nv ? X2[lane] : 0.0, ny2 = nv ? Y2[lane] : 0.0;
        nidx = nv ? (ORDERED ? order[lane] : (uint32_t)lane) : 0;
    }
    for (uint32_t base = 0; base < M; base += W)
    {
        const uint32_t pos = base + lane;
        const bool valid = pos < M;
        const double x1 = nx1, y1 = ny1, x2 = nx2, y2 = ny2;
        const uint32_t idx = nidx;
        {
            const uint32_t np = pos + W;
            const bool nv = np < M;
            nx1 = nv ? X1[np] : 0.0, ny1 = nv ? Y1[np] : 0.0, nx2 = nv ? X2[np] : 0.0, ny2 = nv ? Y2[np] : 0.0;
            nidx = nv ? (ORDERED ? order[np] : np) : 0;
        }
        const double e = model_error(m, x1, y1, x2, y2);
        const bool inl = valid && (e < thr);
        double term = 0;
        if (inl)
        {
            const double ratio = e / thr;
            term = 1.0 - ratio * ratio;
        }
        if (valid)
            flags[idx] = inl ? 1 : 0;
        const unsigned long long mask = __ballot(inl);
        count += __popcll(mask);
        double pref = s; // running sum as seen right after this lane's element
        if (mask)
        {
#pragma unroll
            for (int l = 0; l < W; l++)
            {
                s = s + bcast(term, l);
                if (ORDERED)
                    pref = lane == l ? s : pref;
            }
        }
        if (ORDERED)
        {
            const uint32_t checked = pos + 1;
            const bool rej = valid && checked > 20 && best_score > 0 &&
                             pref < best_score * (double)checked / (double)M * 0.6;
            if (__ballot(rej))
            {
                *rejected = true;
                return s;
            }
        }
    }
    *n_inliers = count;
    return s;
}

// The adaptive iteration count after an improvement (ransac.cpp:247-251) is
//     iterations_needed(log(1 - p) / log(1 - fast_pow<K>(omega))),   omega the score per match:
// the power in the reference's order of products, and static_cast<size_t>(q) clamped to [MIN_ITERATIONS, MAX_ITERATIONS].
template <int K> __device__ __forceinline__ double fast_pow(double x)
{
    static_assert(K == 4 || K == 5 || K == 8, "restated for the three models' sample sizes");
    double t = x * x;
    if (K == 4)
        return t * t;
    if (K == 5)
        return t * t * x;
    t = t * t;
    return t * t;
}
__device__ __forceinline__ uint32_t iterations_needed(double q)
{
    uint64_t qi;
    if (!(q == q)) // NaN -> x86 cvttsd2si gives 0x8000000000000000: huge as size_t
        qi = 0x8000000000000000ull;
    else if (q >= 9223372036854775808.0)
        qi = (q >= 18446744073709551616.0) ? 0ull : (uint64_t)q; // never reached with p = 0.999
    else if (q <= -1.0)
        qi = (uint64_t)(int64_t)q; // negative wraps like the x86 conversion
    else
        qi = (uint64_t)q;
    const uint64_t clamped = qi < MAX_ITERATIONS ? qi : MAX_ITERATIONS;
    return (uint32_t)(clamped > MIN_ITERATIONS ? clamped : MIN_ITERATIONS);
}

} // namespace
