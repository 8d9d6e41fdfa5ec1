// libochip.so — the link stage's RANSAC: homography RANSAC for every image pair of a link batch, one wavefront per pair
// (gfx950), the re-fit of accepted edges, and the tail that turns the results into edges.
//
// Replaces, per directed pair, the whole body of ransac<homography_model> (src/model_inliers/ransac.cpp:53-257): the loop is
// ransac_homography_kernel with its fast_forward, the model-independent parts it calls are ransac_loop.hpp's (shared with
// ransac_epipolar.hip) and homography_model::fit / fitInliers / error / evaluate / checkSampleDegeneracy
// (src/model_inliers/homography_model.cpp:19-136) are homography_fit.hpp's.  Also here: the re-fit of
// RelaxGroup::finalize (src/relax/relax_group.cpp:137-177, refit_homography_kernel), the ray normalisation half of
// distort_keypoints (src/distort/distort_keypoints.cpp:48-103, hoisted to once per image because image_to_3d only depends on
// the keypoint and its camera model), homography_model::decompose (homography_model.cpp:138-185, decompose_vote_kernel), the
// PROSAC order of ransac.cpp:83-90 and the two lists an accepted edge keeps (link_stage.cpp:99-107), with their C entries.
//
// Why one wave per pair: the reference loop is sequential in three places that decide its results
// bit for bit — the minstd_rand0 sample stream, the SPRT early exit that compares a running fp64 MSAC
// sum (in shuffled evaluation order) with the best score so far, and the local-optimisation /
// adaptive-termination chain that follows every improvement.  A wavefront keeps that control flow
// wave-uniform and parallelises inside each step: 64 symmetric-transfer errors per chunk, ballot for
// the SPRT exit and the inlier masks, lane-strided rows for the (2n+1)x9 full-pivot LU of
// fitInliers.  The fp64 score is accumulated strictly in evaluation order (one add per inlier), so
// scores, inlier sets and H are bit-identical to the CPU restatement; pairs are independent, so the
// chip is filled with thousands of resident waves.  All arithmetic is fp64 with -ffp-contract=off
// (the reference is built without FMA); device division and sqrt are correctly rounded
// (tests/test_gpu_fp64.py).  decompose_vote_kernel is held against the host on homographies of known motions through the
// seam ochip_debug_decompose_votes (tests/test_gpu_decompose.py).
#include "homography_fit.hpp"
#include "undistort.hpp"
#include "decompose.hpp"

namespace
{
struct rays_view
{
    const double *rays;      // [total][3]
    const uint64_t *img_off; // per image
};

// ---- fast-forward over iterations that change nothing -------------------------------------------------------------
// An iteration of ransac.cpp:98-247 only touches the state when its model is neither degenerate nor SPRT-rejected and
// scores above the best so far; every other iteration just consumes random numbers.  Link pairs with few matches and
// a low inlier ratio run hundreds to thousands of such iterations (one C3 pair: 6 111, 33 us each when the whole wave
// works on one 9 x 9 fit at a time — that single pair WAS the kernel's duration).  So the next up to FB iterations
// are looked at side by side, one per lane: the sample stream is replayed (uniform, sequential, as it must be), every
// lane fits its own sample with a private 9 x 9 full-pivot LU in LDS and walks the matches in evaluation order with the
// SPRT test, exactly the arithmetic of the one-at-a-time path.  The iterations before the first lane that would
// improve are skipped (rng and PROSAC state advanced past them); that iteration itself then runs on the normal path.
// Returns the number of leading no-op iterations among the next n (rng / prosac_n advanced past them); *found says
// whether the iteration after them would improve the best model (it then runs on the normal path).
__device__ uint32_t fast_forward(const pair_data &pd, const uint32_t *__restrict__ sorted_idx, bool has_quality, uint32_t it,
                                 uint32_t n, uint32_t &rng, uint32_t &prosac_n, double best_score, double thr, double *AQs,
                                 bool *found)
{
    const int lane = threadIdx.x;
    const uint32_t M = pd.M;
    OCHIP_PHASE_COUNT(8, 1);
    OCHIP_PHASE_T0(t_fit);
    // ---- replay the sample stream of the next n iterations (ransac.cpp:104-154, :164-171); lane L keeps iteration it + L
    uint32_t rng_s = rng, prosac_s = prosac_n;
    uint32_t my_rng = 0, my_prosac = 0, my_c[4] = {0, 0, 0, 0};
    for (uint32_t L = 0; L < n; L++)
    {
        const uint32_t itL = it + L, rb = rng_s, pb = prosac_s;
        if (has_quality && prosac_s < M && itL > 0 && itL % 10 == 0) // (prosac_grow, spelled out: see the kernel's sample)
            prosac_s++;
        uint32_t c[4];
        draw_sample<4, false>(rng_s, prosac_s, M, has_quality, nullptr, c);
        if ((uint32_t)lane == L)
        {
            my_rng = rb;
            my_prosac = pb;
            for (int j = 0; j < 4; j++)
                my_c[j] = c[j];
        }
    }
    // ---- every lane: its sample, the degeneracy test, the fit
    const bool active = (uint32_t)lane < n;
    bool live = active;
    model_t m;
    set_nan(m);
    if (active)
    {
        uint32_t s4[4];
        for (int j = 0; j < 4; j++)
            s4[j] = has_quality ? sorted_idx[my_c[j]] : my_c[j];
        double px[4], py[4], qx[4], qy[4];
        for (int j = 0; j < 4; j++)
        {
            px[j] = pd.x1[s4[j]];
            py[j] = pd.y1[s4[j]];
            qx[j] = pd.x2[s4[j]];
            qy[j] = pd.y2[s4[j]];
        }
        if (sample_degenerate(px, py))
            live = false; // the iteration ends here
        if (live)
            lane_fit(AQs + lane, px, py, qx, qy, m);
    }
    OCHIP_PHASE_ADD(t_fit, 1);
    OCHIP_PHASE_T0(t_walk);
    // ---- SPRT-pruned MSAC walk in evaluation order.  The error of a (model, position) is the expensive part (four divisions
    //      and a square root in fp64), the running sum of a model takes its terms one position after the other.  The n <= 32
    //      models sit in lanes 0 .. n - 1; the wave's other lanes evaluate the same models at the following positions - P =
    //      2 .. 4 positions per trip, as many as 64 lanes hold groups of n (19 models, the usual number behind the 20-iteration
    //      floor: 3 positions, 57 lanes busy; rounds 3 - 4 used two half-waves whatever n was) - and hand term and SPRT
    //      limit of their position to the model's lane, which adds and tests them in order.
    static_assert(FB == 32, "two groups of FB models fill the wave");
    const uint32_t P = n > 21 ? 2u : (n > 16 ? 3u : 4u);
    const uint32_t CH = ((uint32_t)W / P) * P; // positions per chunk: whole trips
    const uint32_t slot = ((uint32_t)lane >= n ? 1u : 0u) + ((uint32_t)lane >= 2 * n ? 1u : 0u) + ((uint32_t)lane >= 3 * n ? 1u : 0u);
    const bool evaluates = (uint32_t)lane < P * n;
    const int src = evaluates ? lane - (int)(slot * n) : 0;
    model_t mm;
    for (int i = 0; i < 9; i++)
    {
        mm.H[i] = __shfl(m.H[i], src);
        mm.Hi[i] = __shfl(m.Hi[i], src);
    }
    double s = 0;
    bool rej = false;
    // (round 5: the walk took its four coordinates of every position straight from memory - the same address in all
    // lanes, one L2 round trip per two positions with the exit test between them, 14 k loads per pair and two thirds of the
    // kernel's cycles in s_waitcnt.  Now a chunk of 64 positions is loaded once, a position per lane, and the walk takes a
    // position's coordinates from the lane that holds it: one round trip per chunk, and most walks of a pair with few
    // inliers end inside the first.)
    for (uint32_t base = 0; base < M; base += CH)
    {
        if (__ballot(lane < 32 && live && !rej) == 0)
            break;
        const uint32_t mine = base + (uint32_t)lane;
        const double c_x1 = mine < M ? pd.ex1[mine] : 0.0, c_y1 = mine < M ? pd.ey1[mine] : 0.0;
        const double c_x2 = mine < M ? pd.ex2[mine] : 0.0, c_y2 = mine < M ? pd.ey2[mine] : 0.0;
        const uint32_t chunk_end = min(base + CH, M);
        for (uint32_t pos0 = base; pos0 < chunk_end; pos0 += P)
        {
            if (__ballot(lane < 32 && live && !rej) == 0)
                break;
            const uint32_t pos = pos0 + (evaluates ? slot : 0u);
            const int holder = (int)(pos - base); // (< CH + P - 1 <= 64; a position past the chunk's last is past M or unused)
            const double px1 = __shfl(c_x1, holder), py1 = __shfl(c_y1, holder), px2 = __shfl(c_x2, holder), py2 = __shfl(c_y2, holder);
            double term = 0, limit = 0;
            if (evaluates && pos < chunk_end)
            {
                const double e = transfer_error(mm, px1, py1, px2, py2);
                if (e < thr)
                {
                    const double ratio = e / thr;
                    term = 1.0 - ratio * ratio;
                }
                limit = best_score * (double)(pos + 1) / (double)M * 0.6;
            }
#pragma unroll
            for (uint32_t sl = 0; sl < 4; sl++)
                if (sl < P) // (wave-uniform)
                {
                    const int from = (lane + (int)(sl * n)) & (W - 1);
                    const double t = sl == 0 ? term : __shfl(term, from), lim = sl == 0 ? limit : __shfl(limit, from);
                    if (pos0 + sl < chunk_end)
                    {
                        s = s + t; // position pos0 + sl (lanes 0 .. n - 1; the other lanes' sums are not used)
                        if (pos0 + sl + 1 > 20 && best_score > 0 && s < lim)
                            rej = true;
                    }
                }
        }
    }
    OCHIP_PHASE_ADD(t_walk, 2);
    const unsigned long long improving = __ballot(lane < 32 && live && !rej && s > best_score);
    if (improving == 0)
    {
        rng = rng_s;
        prosac_n = prosac_s;
        *found = false;
        return n;
    }
    const int first = __builtin_ctzll(improving);
    rng = (uint32_t)__builtin_amdgcn_readlane((int)my_rng, first);
    prosac_n = (uint32_t)__builtin_amdgcn_readlane((int)my_prosac, first);
    *found = true;
    return (uint32_t)first;
}

template <int OCC> __global__ __launch_bounds__(W, OCC) __attribute__((amdgpu_num_vgpr(248))) void ransac_homography_kernel(
    const ochip_ransac_job *__restrict__ jobs, const ochip_ransac_match *__restrict__ matches,
    const uint32_t *__restrict__ sorted_idx_all, const uint32_t *__restrict__ eval_order_all, rays_view rv,
    double *__restrict__ coord_scratch /*8 x total*/, uint8_t *__restrict__ flag_scratch /*2 x total*/,
    double *__restrict__ P_scratch /*81 x n_jobs*/, uint64_t total, double thr,
    ochip_ransac_result *__restrict__ results, uint8_t *__restrict__ inliers_out, const uint32_t *__restrict__ launch_order)
{
    __shared__ double P9[81], T9[81], AQs[81 * FB];
    static_assert(sizeof(tall_tab) <= sizeof(double) * 81 * FB, "the factorisation's table borrows the lane fits' LDS");
    const int lane = threadIdx.x;
    const uint32_t job_id = launch_order[blockIdx.x]; // (the pairs with the most matches first: see the launch)
    const ochip_ransac_job job = jobs[job_id];
    const uint32_t M = job.n;
    const uint64_t mo = job.match_offset;

    ochip_ransac_result res = empty_result();
    if (M < 4) // ransac.cpp:67-70
    {
        too_few_matches(res, M, inliers_out + mo, results + job_id);
        return;
    }

    // ---- prologue: gather the unit rays of the matched keypoints, divide by z once (error() and fit()
    //      both start from measurement / measurement.z), detect has_quality (ransac.cpp:74-82); the same
    //      coordinates once more in evaluation order for the SPRT walks
    OCHIP_PHASE_T0(t_total);
    const uint32_t *sorted_idx = sorted_idx_all + mo;
    const uint32_t *eval_order = eval_order_all + job.eval_offset;
    // (the pair's two flag planes trade places on every improvement; the final evaluation writes the caller's array)
    pair_data pd = bind_coords(coord_scratch, total, mo, M);
    const double *r1 = rv.rays + rv.img_off[job.image_1] * 3, *r2 = rv.rays + rv.img_off[job.image_2] * 3;
    bool hq_lane = false;
    for (uint32_t i = lane; i < M; i += W)
    {
        const ochip_ransac_match mt = matches[mo + i];
        const ochip_ransac_match me = matches[mo + eval_order[i]];
        const double ax = r1[(size_t)mt.k1 * 3], ay = r1[(size_t)mt.k1 * 3 + 1], az = r1[(size_t)mt.k1 * 3 + 2];
        const double bx = r2[(size_t)mt.k2 * 3], by = r2[(size_t)mt.k2 * 3 + 1], bz = r2[(size_t)mt.k2 * 3 + 2];
        const double eax = r1[(size_t)me.k1 * 3], eay = r1[(size_t)me.k1 * 3 + 1], eaz = r1[(size_t)me.k1 * 3 + 2];
        const double ebx = r2[(size_t)me.k2 * 3], eby = r2[(size_t)me.k2 * 3 + 1], ebz = r2[(size_t)me.k2 * 3 + 2];
        pd.x1[i] = ax / az;
        pd.y1[i] = ay / az;
        pd.x2[i] = bx / bz;
        pd.y2[i] = by / bz;
        pd.ex1[i] = eax / eaz;
        pd.ey1[i] = eay / eaz;
        pd.ex2[i] = ebx / ebz;
        pd.ey2[i] = eby / ebz;
        hq_lane |= (mt.count != 0); // quality = count * (1/486) != 0  <=>  count != 0
    }
    const bool has_quality = __ballot(hq_lane) != 0;
    __syncthreads();
    OCHIP_PHASE_ADD(t_total, 0);
    bind_scratch<true>(pd, flag_scratch, P_scratch, total, mo, job_id);

    // (the best model lives in LDS: it is written on an improvement and read once at the end, and 36 registers held across
    // the factorisations of the local optimisation were the difference between two wavefronts per SIMD and one)
    __shared__ double best_model_lds[18];
    auto keep_best = [&](const model_t &m) {
        __syncthreads();
        if (lane < 9)
        {
            best_model_lds[lane] = m.H[lane];
            best_model_lds[9 + lane] = m.Hi[lane];
        }
    };
    model_t model;
    set_nan(model);
    keep_best(model);
    double best_score = 0;
    uint32_t rng = job.rng_state;
    uint32_t prosac_n = has_quality ? 4u : M;
    uint32_t probability_iterations = MAX_ITERATIONS;
    const double log_1m_p = log(1 - 0.999);
    uint32_t it = 0;

    for (; it < probability_iterations; it++)
    {
        if (best_score > 0 && probability_iterations - it >= 4)
        {
            // look at the next iterations side by side and skip those that change nothing
            const uint32_t n = min((uint32_t)FB, probability_iterations - it);
            bool found;
            it += fast_forward(pd, sorted_idx, has_quality, it, n, rng, prosac_n, best_score, thr, AQs, &found);
            if (!found)
            {
                it--; // the loop's increment: the next iteration to look at is `it`
                continue;
            }
        }
        if (has_quality)
            prosac_grow(it, prosac_n, M);

        OCHIP_PHASE_T0(t_sample);
        // ---- minimal sample (ransac.cpp:104-154): draw_sample<4, true>, spelled out.  This kernel's code is held to the
        //      instruction, and the call - in any signature tried - comes out of the inliner as other code than
        //      these statements do; so does prosac_grow in the fast-forward's replay.  A change to either goes to both.
        uint32_t s4[4];
        if (has_quality && prosac_n < M && prosac_n > 4)
        {
            uint32_t c[4];
            c[0] = prosac_n - 1; // never drawn again: the other three come from [0, prosac_n - 2]
            draw_distinct<4>(rng, prosac_n - 2, 1, c);
            for (int j = 0; j < 4; j++)
                s4[j] = sorted_idx[c[j]];
        }
        else
        {
            uint32_t c[4];
            draw_distinct<4>(rng, (has_quality ? prosac_n : M) - 1, 0, c);
            for (int j = 0; j < 4; j++)
                s4[j] = has_quality ? sorted_idx[c[j]] : c[j];
        }

        // ---- checkSampleDegeneracy (homography_model.cpp:120-136) on measurement1.hnormalized()
        double px[4], py[4], qx[4], qy[4];
        for (int j = 0; j < 4; j++)
        {
            px[j] = pd.x1[s4[j]];
            py[j] = pd.y1[s4[j]];
            qx[j] = pd.x2[s4[j]];
            qy[j] = pd.y2[s4[j]];
        }
        if (sample_degenerate(px, py))
            continue;

        // ---- fit (homography_model.cpp:19-50): 9x9 DLT system in LDS
        __syncthreads();
        if (lane < 4)
            write_dlt_rows(P9, 9, 2 * lane, px[lane], py[lane], qx[lane], qy[lane]);
        if (lane < 9)
            P9[lane * 9 + 8] = lane == 8 ? 1.0 : 0.0;
        double sol[9];
        full_piv_lu_solve9(P9, 9, sol);
        model_from_solution(model, sol);
        OCHIP_PHASE_ADD(t_sample, 3);

        // ---- SPRT-pruned MSAC scoring in shuffled order (ransac.cpp:181-205)
        bool rejected;
        uint32_t n_inl = 0;
        OCHIP_PHASE_T0(t_score);
        const double score = score_walk<true>(model, pd, eval_order, pd.cand, thr, best_score, &rejected, &n_inl);
        OCHIP_PHASE_ADD(t_score, 4);
        OCHIP_PHASE_COUNT(9, 1);
        if (rejected)
            continue;

        if (score > best_score)
        {
            res.improvements++;
            keep_best(model);
            best_score = score;
            __syncthreads();
            {
                uint8_t *t = pd.cand; // inliers = candidate flags of this model
                pd.cand = pd.inl;
                pd.inl = t;
            }
            uint32_t n_in = n_inl; // the scoring was not cut short, so it counted every inlier it flagged

            // local optimisation: fitInliers + evaluate, up to MAX_INNER_ITERATIONS (ransac.cpp:224-245)
            for (uint32_t j = 0; j < MAX_INNER_ITERATIONS; j++)
            {
                OCHIP_PHASE_T0(t_fi);
                fit_inliers(pd, n_in, T9, reinterpret_cast<tall_tab *>(AQs), model); // (the lane fits' LDS is idle here)
                OCHIP_PHASE_ADD(t_fi, 5);
                OCHIP_PHASE_COUNT(10, 1);
                bool dummy;
                uint32_t cnt = 0;
                __syncthreads();
                OCHIP_PHASE_T0(t_sf);
                const double inlier_score = score_walk<false>(model, pd, nullptr, pd.inl, thr, 0.0, &dummy, &cnt);
                __syncthreads();
                OCHIP_PHASE_ADD(t_sf, 6);
                n_in = cnt;
                if (inlier_score > best_score)
                {
                    keep_best(model);
                    best_score = inlier_score;
                }
                else
                    break;
            }

            const double omega = best_score / (double)M;
            const double omega_n = fast_pow<4>(omega);
            const double log_1m_omega_n = log(1 - omega_n);
            probability_iterations = iterations_needed(log_1m_p / log_1m_omega_n);
        }
    }

    // ---- model = best_model; return model.evaluate(matches, inliers) / matches.size()
    bool dummy;
    uint32_t cnt = 0;
    __syncthreads();
    for (int i = 0; i < 9; i++)
    {
        model.H[i] = best_model_lds[i];
        model.Hi[i] = best_model_lds[9 + i];
    }
    const double final_score = score_walk<false>(model, pd, nullptr, inliers_out + mo, thr, 0.0, &dummy, &cnt);
    for (int i = 0; i < 9; i++)
        res.H[i] = model.H[i];
    res.score = final_score / (double)M;
    res.iterations = it;
    res.n_inliers = cnt;
    if (lane == 0)
        results[job_id] = res;
    OCHIP_PHASE_ADD(t_total, 7);
    OCHIP_PHASE_COUNT(11, res.improvements);
#ifdef OCHIP_RANSAC_PHASES
    if (threadIdx.x == 0)
    {
        const unsigned long long mine = clock64() - t_total;
        atomicMax(&g_phase[13], mine);
        if (mine > 20000000ull)
            atomicAdd(&g_phase[14], 1ull);
        if (mine > 10000000ull)
            atomicAdd(&g_phase[15], 1ull);
    }
#endif
}

// ---- re-fit of an edge's homography on its previous inliers after the camera models changed
//      (RelaxGroup::finalize, src/relax/relax_group.cpp:137-177): rays from the current models, then `rounds` times
//      fitInliers + evaluate starting from the previous inlier set.  One wavefront per edge, the RANSAC kernel's
//      device functions.
__global__ __launch_bounds__(W, 2) __attribute__((amdgpu_num_vgpr(248))) void refit_homography_kernel(
    const ochip_ransac_job *__restrict__ jobs, const ochip_ransac_match *__restrict__ matches, rays_view rv,
    double *__restrict__ coord_scratch /*4 x total*/, double *__restrict__ P_scratch /*81 x n_jobs*/, uint64_t total,
    double thr, uint32_t rounds, ochip_ransac_result *__restrict__ results, uint8_t *__restrict__ inliers /*in: previous, out: new*/)
{
    __shared__ double T9[81];
    __shared__ tall_tab tall;
    const int lane = threadIdx.x;
    const uint32_t job_id = blockIdx.x;
    const ochip_ransac_job job = jobs[job_id];
    const uint32_t M = job.n;
    const uint64_t mo = job.match_offset;
    pair_data pd = bind_coords(coord_scratch, total, mo, M);
    pd.ex1 = pd.ey1 = pd.ex2 = pd.ey2 = nullptr; // (a refit has no evaluation order, and its scratch is 4 x total)
    const double *r1 = rv.rays + rv.img_off[job.image_1] * 3, *r2 = rv.rays + rv.img_off[job.image_2] * 3;
    uint32_t n_in = 0;
    for (uint32_t base = 0; base < M; base += W)
    {
        const uint32_t i = base + lane;
        bool f = false;
        if (i < M)
        {
            const ochip_ransac_match mt = matches[mo + i];
            const double ax = r1[(size_t)mt.k1 * 3], ay = r1[(size_t)mt.k1 * 3 + 1], az = r1[(size_t)mt.k1 * 3 + 2];
            const double bx = r2[(size_t)mt.k2 * 3], by = r2[(size_t)mt.k2 * 3 + 1], bz = r2[(size_t)mt.k2 * 3 + 2];
            pd.x1[i] = ax / az;
            pd.y1[i] = ay / az;
            pd.x2[i] = bx / bz;
            pd.y2[i] = by / bz;
            f = inliers[mo + i] != 0;
        }
        n_in += __popcll(__ballot(f));
    }
    __syncthreads();
    pd.inl = inliers + mo;
    bind_scratch<false>(pd, nullptr, P_scratch, total, mo, job_id);
    model_t model;
    set_nan(model);
    double score = 0;
    uint32_t cnt = n_in;
    for (uint32_t r = 0; r < rounds; r++)
    {
        fit_inliers(pd, cnt, T9, &tall, model);
        bool dummy;
        __syncthreads();
        score = score_walk<false>(model, pd, nullptr, pd.inl, thr, 0.0, &dummy, &cnt);
        __syncthreads();
    }
    ochip_ransac_result res;
    for (int i = 0; i < 9; i++)
        res.H[i] = model.H[i];
    res.score = M ? score / (double)M : 0.0;
    res.iterations = rounds;
    res.n_inliers = cnt;
    res.improvements = 0;
    res.reserved = 0;
    if (lane == 0)
        results[job_id] = res;
}

// ---- test seam: homography_model::fit of given minimal samples through the two device routes that have no entry of their
//      own (include/ochip.h: ochip_debug_homography_fit4, tests/test_gpu_homography_fit.py).  ROUTE 0: one wavefront per
//      sample, the 9 x 9 system in LDS and the wave-cooperative full_piv_lu_solve9 - the statements of the RANSAC loop's
//      normal path; ROUTE 1: FB samples per wavefront, lane_fit on the fast-forward's interleaved LDS layout.  The fit runs
//      whatever checkSampleDegeneracy says (the loop would skip the sample); its answer is returned beside it.
template <int ROUTE>
__global__ __launch_bounds__(W) void debug_fit4_kernel(const double *__restrict__ xy16, uint32_t n, double *__restrict__ H9,
                                                       double *__restrict__ Hinv9, uint8_t *__restrict__ degenerate_out)
{
    __shared__ double LDS[ROUTE == 0 ? 81 : 81 * FB];
    const int lane = threadIdx.x;
    const uint32_t s = ROUTE == 0 ? blockIdx.x : blockIdx.x * FB + (uint32_t)lane;
    const bool active = s < n && (ROUTE == 0 || lane < FB);
    double px[4], py[4], qx[4], qy[4];
    for (int j = 0; j < 4; j++)
    {
        px[j] = active ? xy16[(size_t)s * 16 + 4 * j] : 0.0;
        py[j] = active ? xy16[(size_t)s * 16 + 4 * j + 1] : 0.0;
        qx[j] = active ? xy16[(size_t)s * 16 + 4 * j + 2] : 0.0;
        qy[j] = active ? xy16[(size_t)s * 16 + 4 * j + 3] : 0.0;
    }
    const bool degenerate = sample_degenerate(px, py);
    model_t model;
    set_nan(model);
    if (ROUTE == 0)
    {
        if (!active) // (wave-uniform: the grid is one block per sample)
            return;
        if (lane < 4)
            write_dlt_rows(LDS, 9, 2 * lane, px[lane], py[lane], qx[lane], qy[lane]);
        if (lane < 9)
            LDS[lane * 9 + 8] = lane == 8 ? 1.0 : 0.0;
        double sol[9];
        full_piv_lu_solve9(LDS, 9, sol);
        model_from_solution(model, sol);
    }
    else if (active)
        lane_fit(LDS + lane, px, py, qx, qy, model);
    if (active && (ROUTE == 1 || lane == 0))
    {
        for (int i = 0; i < 9; i++)
        {
            H9[(size_t)s * 9 + i] = model.H[i];
            Hinv9[(size_t)s * 9 + i] = model.Hi[i];
        }
        degenerate_out[s] = degenerate ? 1 : 0;
    }
}

// pixel -> unit ray, distort_keypoints.cpp:68-103 (csrc/undistort.hpp: lens distortion is inverted per keypoint with
// the restated TinySolver; one thread per keypoint, the solver's <= 10 iterations are a few hundred flops)
__global__ void keypoints_to_rays_kernel(const double *__restrict__ xy, const double *__restrict__ models /*[img][8]*/,
                                         const uint32_t *__restrict__ kp_image, double *__restrict__ rays, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const double *m = models + (size_t)kp_image[i] * 8;
    double model8[8], kp[2] = {xy[2 * i], xy[2 * i + 1]}, ray[3];
    for (int k = 0; k < 8; k++)
        model8[k] = m[k];
    ochip_ud::image_to_3d(kp, model8, ray);
    rays[3 * i] = ray[0];
    rays[3 * i + 1] = ray[1];
    rays[3 * i + 2] = ray[2];
}

} // namespace

extern "C"
{

int ochip_upload_keypoints(ochip_ctx *ctx, uint32_t image_id, const double *xy, uint32_t n, const double *model8)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (image_id >= ctx->n_images || !ctx->img_set[image_id])
        return ochip_fail(ctx, OCHIP_ESTATE, "upload the descriptors of image %u first", image_id);
    if (n != ctx->img_n[image_id])
        return ochip_fail(ctx, OCHIP_EINVAL, "image %u: %u keypoints but %u descriptors", image_id, n,
                          ctx->img_n[image_id]);
    if (!model8 || (n && !xy))
        return ochip_fail(ctx, OCHIP_EINVAL, "NULL argument");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->kp_store_ready)
    {
        const int rc = ochip_ensure_keypoint_store(ctx, ctx->desc_capacity, ctx->n_images);
        if (rc)
            return rc;
        ctx->kp_set.assign(ctx->n_images, 0);
    }
    const uint64_t off = ctx->img_off[image_id];
    std::vector<uint32_t> ids(n, image_id);
    if (n)
    {
        OCHIP_HIP(ctx, hipMemcpyAsync(ctx->kp_xy_dev + 2 * off, xy, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(ctx->kp_image_dev + off, ids.data(), (size_t)n * 4, hipMemcpyHostToDevice,
                                      ctx->stream));
    }
    OCHIP_HIP(ctx, hipMemcpyAsync(ctx->models_dev + (size_t)image_id * 8, model8, 64, hipMemcpyHostToDevice,
                                  ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    ctx->kp_set[image_id] = 1;
    ctx->rays_dirty = true;
    return OCHIP_OK;
}

} // extern "C"

namespace
{
// matches of job j out of ochip_match_sort's records: correspondence i = the i-th sorted record of the pair; and the keys
// of the PROSAC order (ransac.cpp:83-90: iota sorted by quality ASCENDING with std::sort - complemented counts)
__global__ void sorted_matches_kernel(const ochip_ransac_job *__restrict__ jobs, const unsigned int *__restrict__ seg_begin,
                                      const unsigned long long *__restrict__ recs, const ochip_match *__restrict__ raw,
                                      ochip_ransac_match *__restrict__ matches, unsigned long long *__restrict__ prosac,
                                      unsigned int *__restrict__ seg2)
{
    const unsigned int j = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    const ochip_ransac_job jb = jobs[j];
    if (i == 0)
    {
        seg2[j] = (unsigned int)jb.match_offset;
        seg2[gridDim.y + j] = (unsigned int)jb.match_offset + jb.n;
    }
    if (i >= jb.n)
        return;
    const unsigned int off = seg_begin[j];
    const unsigned long long r = recs[off + i];
    const unsigned int a = (unsigned int)r, count = (unsigned int)(r >> 32);
    ochip_ransac_match m;
    m.k1 = a;
    m.k2 = raw[off + a].best_k;
    m.count = (uint16_t)count;
    m.reserved = 0;
    matches[jb.match_offset + i] = m;
    prosac[jb.match_offset + i] = ((unsigned long long)(0xFFFFFFFFu - count) << 32) | i;
}
// homography_model::decompose (homography_model.cpp:138-185) for every job: cv::decomposeHomographyMat by one lane
// (csrc/decompose.hpp, the host's code), the cheirality vote over the inliers' rays by the wavefront (integers: the order is
// free), the poses in std::stable_sort's order.  One wavefront per job.
__global__ __launch_bounds__(256) void decompose_vote_kernel(const ochip_ransac_job *__restrict__ jobs, unsigned int n_jobs,
                                                             const ochip_ransac_match *__restrict__ matches,
                                                             const ochip_ransac_result *__restrict__ results,
                                                             const uint8_t *__restrict__ inliers, rays_view rv,
                                                             ochip_decomposition *__restrict__ out)
{
    __shared__ ochip_dc::vote_plan plans[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned int j = blockIdx.x * 4 + wv;
    if (j >= n_jobs)
        return;
    const ochip_ransac_job jb = jobs[j];
    ochip_dc::vote_plan &plan = plans[wv];
    if (lane == 0)
        ochip_dc::plan_votes(results[j].H, &plan);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int solutions = plan.solutions;
    const double *r1 = rv.rays + rv.img_off[jb.image_1] * 3, *r2 = rv.rays + rv.img_off[jb.image_2] * 3;
    const ochip_ransac_match *mm = matches + jb.match_offset;
    const uint8_t *inl = inliers + jb.match_offset;
    int votes[4] = {0, 0, 0, 0};
    unsigned int n_inl = 0;
    for (unsigned int i0 = 0; i0 < jb.n; i0 += 64)
    {
        const unsigned int i = i0 + lane;
        const bool on = i < jb.n && inl[i] != 0;
        bool ok[4] = {false, false, false, false};
        if (on)
        {
            const double *m1 = r1 + 3 * (size_t)mm[i].k1, *m2 = r2 + 3 * (size_t)mm[i].k2;
            const double a0 = m1[0], a1 = m1[1], a2 = m1[2], b0 = m2[0], b1 = m2[1], b2 = m2[2];
            for (int s = 0; s < 4; s++)
                if (s < solutions)
                {
                    const double dot1 = plan.N[s][0] * a0 + plan.N[s][1] * a1 + plan.N[s][2] * a2;
                    const double dot2 = plan.RN[s][0] * b0 + plan.RN[s][1] * b1 + plan.RN[s][2] * b2;
                    ok[s] = dot1 >= 0 && dot2 >= 0;
                }
        }
        n_inl += (unsigned int)__popcll(__ballot(on));
        for (int s = 0; s < 4; s++)
            votes[s] += (int)__popcll(__ballot(ok[s]));
    }
    if (lane == 0)
    {
        int score[4], order[4];
        for (int s = 0; s < 4; s++)
            score[s] = s < solutions ? votes[s] : -1;
        ochip_dc::order_by_votes(score, order);
        ochip_decomposition d;
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
        for (int k = 0; k < 4; k++)
        {
            const int s = order[k];
            for (int c = 0; c < 4; c++)
                d.pose[k][c] = s < solutions ? plan.q[s][c] : nan;
            for (int c = 0; c < 3; c++)
                d.pose[k][4 + c] = s < solutions ? plan.t[s][c] : nan;
            d.pose[k][7] = (double)score[s];
        }
        d.can_decompose = score[order[0]] > 0 ? 1u : 0u;
        d.n_inliers = n_inl;
        out[j] = d;
    }
}

// The two lists an accepted edge keeps (camera_relations.matches and .inlier_matches, link_stage.cpp:99-107): pure gathers
// of what the device holds - the sorted correspondences, the inlier flags, the subsets' pixel locations and the
// keypoints' indices in their images' feature lists.  One wavefront per job; inliers in match order (ballot prefix).
struct edge_feature_match // types/feature_match.hpp:11-23
{
    uint64_t feature_index_1, feature_index_2;
    double distance;
};
struct edge_inlier_match // types/feature_match.hpp:26-39 (feature_match_denormalized)
{
    double pixel_1[2], pixel_2[2];
    uint64_t feature_index_1, feature_index_2, match_index;
};
__global__ __launch_bounds__(256) void edge_lists_kernel(const ochip_ransac_job *__restrict__ jobs, unsigned int n_jobs,
                                                         const ochip_ransac_match *__restrict__ matches,
                                                         const uint8_t *__restrict__ inliers, const uint64_t *__restrict__ img_off,
                                                         const double *__restrict__ kp_xy, const uint32_t *__restrict__ feature_index,
                                                         const uint64_t *__restrict__ inlier_offset, edge_feature_match *__restrict__ fm,
                                                         edge_inlier_match *__restrict__ fmd)
{
    const int lane = threadIdx.x & 63;
    const unsigned int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_jobs)
        return;
    const ochip_ransac_job jb = jobs[j];
    const uint64_t o1 = img_off[jb.image_1], o2 = img_off[jb.image_2];
    const ochip_ransac_match *mm = matches + jb.match_offset;
    const uint8_t *inl = inliers + jb.match_offset;
    uint64_t at = inlier_offset[j];
    for (unsigned int i0 = 0; i0 < jb.n; i0 += 64)
    {
        const unsigned int i = i0 + lane;
        bool on = false;
        ochip_ransac_match m{};
        uint64_t f1 = 0, f2 = 0;
        if (i < jb.n)
        {
            m = mm[i];
            f1 = feature_index[o1 + m.k1];
            f2 = feature_index[o2 + m.k2];
            edge_feature_match r;
            r.feature_index_1 = f1;
            r.feature_index_2 = f2;
            r.distance = (double)m.count * (1.0 / 486); // count * (1.0 / feature_2d::DESCRIPTOR_BITS), match_features.cpp:90
            fm[jb.match_offset + i] = r;
            on = inl[i] != 0;
        }
        const unsigned long long mask = __ballot(on);
        if (on)
        {
            edge_inlier_match r;
            const double *p1 = kp_xy + 2 * (o1 + m.k1), *p2 = kp_xy + 2 * (o2 + m.k2);
            r.pixel_1[0] = p1[0], r.pixel_1[1] = p1[1];
            r.pixel_2[0] = p2[0], r.pixel_2[1] = p2[1];
            r.feature_index_1 = f1;
            r.feature_index_2 = f2;
            r.match_index = i;
            fmd[at + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull))] = r;
        }
        at += (uint64_t)__popcll(mask);
    }
}

__global__ void prosac_order_kernel(const unsigned long long *__restrict__ prosac, uint32_t *__restrict__ sorted_idx, uint64_t total)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total)
        sorted_idx[i] = (uint32_t)prosac[i];
}

// What the homography entries do before they size the scratch: the jobs against the keypoint store (eval_total == nullptr: the
// jobs have no evaluation order), the rays if a keypoint or a model changed, the image tables.
int prepare_homography_jobs(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, uint64_t total_matches, const uint64_t *eval_total)
{
    for (uint32_t j = 0; j < n_jobs; j++)
    {
        const ochip_ransac_job &jb = jobs[j];
        if (jb.image_1 >= ctx->n_images || jb.image_2 >= ctx->n_images || !ctx->kp_set[jb.image_1] || !ctx->kp_set[jb.image_2])
            return ochip_fail(ctx, OCHIP_ESTATE, "job %u references an image without keypoints", j);
        if (jb.match_offset + jb.n > total_matches || (eval_total && jb.eval_offset + jb.n > *eval_total))
            return ochip_fail(ctx, OCHIP_EINVAL, "job %u: offsets exceed the arrays", j);
    }
    if (ctx->rays_dirty)
    {
        const uint64_t n = ctx->desc_used;
        if (n)
            hipLaunchKernelGGL(keypoints_to_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->kp_xy_dev,
                               ctx->models_dev, ctx->kp_image_dev, ctx->rays_dev, n);
        OCHIP_HIP(ctx, hipGetLastError());
        ctx->rays_dirty = false;
    }
    return ochip_upload_image_tables(ctx);
}

const char *writer_name(ochip::ransac_writer w)
{
    static const char *const names[] = {"no call", "ochip_ransac_homography_batch", "ochip_ransac_homography_batch_sorted",
                                        "ochip_refit_homography_batch", "ochip_ransac_epipolar_batch"};
    return names[(int)w];
}

int ransac_homography_impl(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, const ochip_ransac_match *matches,
                           const uint32_t *sorted_idx, uint64_t total_matches, const uint32_t *eval_order, uint64_t eval_total,
                           double inlier_threshold, ochip_ransac_result *results, uint8_t *inliers, bool sorted_on_device,
                           ochip_ransac_match *matches_out, uint8_t *fallback_out, ochip_decomposition *decomp_out);
} // namespace

int ochip::ransac_scratch::ensure(ochip_ctx *ctx, ransac_writer who, uint32_t n_jobs, size_t job_bytes, uint64_t T, size_t corr_bytes,
                                  uint64_t eval_total, unsigned flags_per_corr)
{
    last = who;
    const bool search = flags_per_corr != 0; // (a refit samples nothing: no orders, no flags of a hypothesis)
    OCHIP_TRY(jobs.ensure(ctx, n_jobs * job_bytes));
    OCHIP_TRY(corr.ensure(ctx, T * corr_bytes));
    OCHIP_TRY(prosac.ensure(ctx, search ? T : 0));
    OCHIP_TRY(eval_order.ensure(ctx, search ? (eval_total ? eval_total : 1) : 0));
    OCHIP_TRY(coords.ensure(ctx, T * 8));
    OCHIP_TRY(flags.ensure(ctx, T * flags_per_corr));
    OCHIP_TRY(lu.ensure(ctx, (size_t)n_jobs * 81));
    return out.ensure(ctx, n_jobs * sizeof(ochip_ransac_result) + T);
}

extern "C"
{

int ochip_ransac_homography_batch(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs,
                                  const ochip_ransac_match *matches, const uint32_t *sorted_idx, uint64_t total_matches,
                                  const uint32_t *eval_order, uint64_t eval_total, double inlier_threshold,
                                  ochip_ransac_result *results, uint8_t *inliers)
{
    return ransac_homography_impl(ctx, jobs, n_jobs, matches, sorted_idx, total_matches, eval_order, eval_total, inlier_threshold,
                                  results, inliers, false, nullptr, nullptr, nullptr);
}

int ochip_ransac_homography_batch_sorted(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, uint64_t total_matches,
                                         const uint32_t *eval_order, uint64_t eval_total, double inlier_threshold,
                                         ochip_ransac_result *results, uint8_t *inliers, ochip_ransac_match *matches_out,
                                         uint8_t *fallback_out, ochip_decomposition *decomp_out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (n_jobs && (!matches_out || !fallback_out))
        return ochip_fail(ctx, OCHIP_EINVAL, "NULL argument");
    if (n_jobs != ctx->ms_pairs)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_ransac_homography_batch_sorted must follow ochip_match_sort of the same %u pairs", n_jobs);
    return ransac_homography_impl(ctx, jobs, n_jobs, nullptr, nullptr, total_matches, eval_order, eval_total, inlier_threshold, results,
                                  inliers, true, matches_out, fallback_out, decomp_out);
}

} // extern "C"

namespace
{
int ransac_homography_impl(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, const ochip_ransac_match *matches,
                           const uint32_t *sorted_idx, uint64_t total_matches, const uint32_t *eval_order, uint64_t eval_total,
                           double inlier_threshold, ochip_ransac_result *results, uint8_t *inliers, bool sorted_on_device,
                           ochip_ransac_match *matches_out, uint8_t *fallback_out, ochip_decomposition *decomp_out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (n_jobs == 0)
        return OCHIP_OK;
    if (!jobs || !results || (total_matches && ((!sorted_on_device && (!matches || !sorted_idx)) || !inliers)) || (eval_total && !eval_order))
        return ochip_fail(ctx, OCHIP_EINVAL, "NULL argument");
    if (!ctx->kp_store_ready)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_upload_keypoints has not been called");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    OCHIP_TRY(prepare_homography_jobs(ctx, jobs, n_jobs, total_matches, &eval_total));
    const uint64_t T = total_matches ? total_matches : 1;
    ochip::ransac_scratch &rs = ctx->ransac;
    OCHIP_TRY(rs.ensure(ctx, sorted_on_device ? ochip::ransac_writer::homography_batch_sorted : ochip::ransac_writer::homography_batch, n_jobs,
                        sizeof(ochip_ransac_job), T, sizeof(ochip_ransac_match), eval_total, 2));
    const ochip_ransac_job *jobs_dev = rs.jobs.as<ochip_ransac_job>();
    ochip_ransac_match *matches_dev = rs.corr.as<ochip_ransac_match>();
    OCHIP_HIP(ctx, hipMemcpyAsync(rs.jobs, jobs, (size_t)n_jobs * sizeof(ochip_ransac_job), hipMemcpyHostToDevice, ctx->stream));
    // (an early error return can leave kernels in flight that still touch these blocks: dev_scratch waits for the stream before
    // it hands them back; the normal path releases them after its own wait at the end)
    ochip::dev_scratch mem{ctx, "ochip_ransac_homography_batch"};
    if (total_matches && !sorted_on_device)
    {
        OCHIP_HIP(ctx, hipMemcpyAsync(matches_dev, matches, (size_t)total_matches * sizeof(ochip_ransac_match), hipMemcpyHostToDevice,
                                      ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(rs.prosac, sorted_idx, (size_t)total_matches * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    else if (total_matches)
    {
        // the correspondences out of ochip_match_sort's records, and their PROSAC order by the same device std::sort
        if (total_matches >= 0xFFFFFFFFull)
            return ochip_fail(ctx, OCHIP_EINVAL, "more than 2^32 matches in one batch");
        uint32_t max_n = 0;
        for (uint32_t j = 0; j < n_jobs; j++)
            max_n = std::max(max_n, jobs[j].n);
        unsigned long long *prosac = (unsigned long long *)mem.get((size_t)total_matches * 8);
        unsigned int *seg2 = (unsigned int *)mem.get((size_t)n_jobs * 8);
        unsigned char *fb2 = (unsigned char *)mem.get(n_jobs);
        if (!prosac || !seg2 || !fb2)
            return OCHIP_ENOMEM;
        hipLaunchKernelGGL(sorted_matches_kernel, dim3((max_n + 255) / 256, n_jobs), dim3(256), 0, ctx->stream, jobs_dev,
                           ctx->ms_seg_dev.as<unsigned int>(), ctx->ms_recs_dev, ctx->match_out_dev, matches_dev, prosac, seg2);
        const int src = ochip::std_sort_enqueue(ctx, mem, prosac, total_matches, seg2, seg2 + n_jobs, n_jobs, max_n, fb2);
        if (src != OCHIP_OK)
            return src;
        hipLaunchKernelGGL(prosac_order_kernel, dim3((unsigned)((total_matches + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const unsigned long long *)prosac, rs.prosac, total_matches);
        OCHIP_HIP(ctx, hipMemcpyAsync(matches_out, matches_dev, (size_t)total_matches * sizeof(ochip_ransac_match),
                                      hipMemcpyDeviceToHost, ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(fallback_out, fb2, n_jobs, hipMemcpyDeviceToHost, ctx->stream));
    }
    else if (sorted_on_device)
        for (uint32_t j = 0; j < n_jobs; j++)
            fallback_out[j] = 0;
    if (eval_total)
        OCHIP_HIP(ctx, hipMemcpyAsync(rs.eval_order, eval_order, (size_t)eval_total * 4, hipMemcpyHostToDevice, ctx->stream));
    rays_view rv{ctx->rays_dev, ctx->img_off_dev};
    const ochip::ransac_scratch::outputs out = rs.outputs_of(n_jobs);
    // A pair is one wavefront from its first sample to its last evaluation, 2 048 of them at a time, and what a pair costs
    // goes with its matches (every scoring, walk and factorisation is a sweep over them): taken in the caller's order the
    // launch ended with a few long pairs that had started late - 17.3 ms for 9 000 pairs whose work fills the device for
    // 9.8.  Longest first.
    uint32_t *order_dev = nullptr;
    std::vector<uint32_t> order(n_jobs); // (read by the copy below until the stream wait at the end)
    {
        for (uint32_t j = 0; j < n_jobs; j++)
            order[j] = j;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].n > jobs[b].n; });
        order_dev = (uint32_t *)mem.get((size_t)n_jobs * 4);
        if (!order_dev)
            return OCHIP_ENOMEM;
        OCHIP_HIP(ctx, hipMemcpyAsync(order_dev, order.data(), (size_t)n_jobs * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    hipEvent_t e0, e1;
    ochip_prof_begin(ctx, OCHIP_K_RANSAC, &e0, &e1);
    // the wave keeps two models, a sample and the LU rows of a round in VGPRs (uniform fp64 values have no scalar
    // home on gfx950): 2 waves per SIMD leaves it 256 registers, 1 leaves it 512 (measured slower)
    constexpr int occ = 2;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(n_jobs), dim3(W), 0, ctx->stream, jobs_dev, matches_dev, rs.prosac, rs.eval_order, rv, rs.coords,
                           rs.flags, rs.lu, (uint64_t)T, inlier_threshold, out.results, out.inliers, (const uint32_t *)order_dev);
    };
    static_assert(occ == 2, "the kernel's register cap is written for two wavefronts per SIMD");
    launch(ransac_homography_kernel<2>);
    ochip_prof_end(ctx, OCHIP_K_RANSAC, e0, e1);
    OCHIP_HIP(ctx, hipGetLastError());
#ifdef OCHIP_RANSAC_PHASES
    {
        unsigned long long ph[16], zero[16] = {};
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_phase), sizeof ph));
        OCHIP_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_phase), zero, sizeof zero));
        static const char *names[13] = {"prologue", "ff replay + fits", "ff walk", "sample + fit", "score (SPRT)", "fit_inliers", "score (inliers)", "total",
                                        "ff calls", "scored iterations", "inner iterations", "improvements", "plain-division trips"};
        std::fprintf(stderr, "ransac phases, %u pairs:", n_jobs);
        for (int i = 0; i < 13; i++)
            std::fprintf(stderr, " %s %.3g%s", names[i], i < 8 ? (double)ph[i] / (double)ph[7] : (double)ph[i] / n_jobs, i < 8 ? "" : "/pair");
        std::fprintf(stderr, "; total %.0f clocks per pair, slowest pair %.0f, pairs over 20 M clocks %llu, over 10 M %llu\n", (double)ph[7] / n_jobs, (double)ph[13], ph[14], ph[15]);
    }
#endif
    if (decomp_out)
    {
        ochip_decomposition *dec_dev = (ochip_decomposition *)mem.get((size_t)n_jobs * sizeof(ochip_decomposition));
        if (!dec_dev)
            return OCHIP_ENOMEM;
        hipLaunchKernelGGL(decompose_vote_kernel, dim3((n_jobs + 3) / 4), dim3(256), 0, ctx->stream, jobs_dev, n_jobs, matches_dev, out.results,
                           out.inliers, rv, dec_dev);
        OCHIP_HIP(ctx, hipMemcpyAsync(decomp_out, dec_dev, (size_t)n_jobs * sizeof(ochip_decomposition), hipMemcpyDeviceToHost,
                                      ctx->stream));
    }
    OCHIP_HIP(ctx, hipMemcpyAsync(results, out.results, (size_t)n_jobs * sizeof(ochip_ransac_result), hipMemcpyDeviceToHost,
                                  ctx->stream));
    if (total_matches)
        OCHIP_HIP(ctx, hipMemcpyAsync(inliers, out.inliers, (size_t)total_matches, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    mem.release();
    for (uint32_t j = 0; j < n_jobs; j++)
        ctx->ransac_hyp_corr += (uint64_t)results[j].iterations * jobs[j].n;
    return OCHIP_OK;
}
} // namespace

extern "C"
{

int ochip_edge_lists(ochip_ctx *ctx, uint32_t n_jobs, uint64_t total_matches, const uint32_t *feature_index, uint64_t n_keypoints,
                     const uint64_t *inlier_offset, uint64_t total_inliers, void *feature_match_out, void *inlier_match_out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (n_jobs == 0)
        return OCHIP_OK;
    if (!feature_index || !inlier_offset || (total_matches && !feature_match_out) || (total_inliers && !inlier_match_out))
        return ochip_fail(ctx, OCHIP_EINVAL, "NULL argument");
    // the kernel gathers through the jobs, correspondences and inlier flags that entry left in the scratch: any other RANSAC
    // call on the context since then has put its own there
    if (ctx->ransac.last != ochip::ransac_writer::homography_batch_sorted)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_edge_lists must follow ochip_ransac_homography_batch_sorted; the RANSAC scratch was last written by %s",
                          writer_name(ctx->ransac.last));
    if (n_jobs != ctx->ms_pairs || n_keypoints != ctx->desc_used)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_edge_lists must follow ochip_ransac_homography_batch_sorted of the same batch");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ochip::dev_scratch mem{ctx, "ochip_edge_lists"};
    uint32_t *idx_dev = (uint32_t *)mem.get((size_t)n_keypoints * 4);
    uint64_t *off_dev = (uint64_t *)mem.get((size_t)n_jobs * 8);
    edge_feature_match *fm_dev = (edge_feature_match *)mem.get((size_t)total_matches * sizeof(edge_feature_match));
    edge_inlier_match *fmd_dev = (edge_inlier_match *)mem.get((size_t)total_inliers * sizeof(edge_inlier_match));
    int rc = idx_dev && off_dev && fm_dev && fmd_dev ? OCHIP_OK : OCHIP_ENOMEM;
    if (rc == OCHIP_OK && (hipMemcpyAsync(idx_dev, feature_index, (size_t)n_keypoints * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
                           hipMemcpyAsync(off_dev, inlier_offset, (size_t)n_jobs * 8, hipMemcpyHostToDevice, st) != hipSuccess))
        rc = ochip_fail(ctx, OCHIP_EHIP, "upload failed (edge lists)");
    if (rc == OCHIP_OK)
    {
        const ochip::ransac_scratch &rs = ctx->ransac;
        hipLaunchKernelGGL(edge_lists_kernel, dim3((n_jobs + 3) / 4), dim3(256), 0, st, rs.jobs.as<ochip_ransac_job>(), n_jobs,
                           rs.corr.as<ochip_ransac_match>(), rs.outputs_of(n_jobs).inliers, ctx->img_off_dev, ctx->kp_xy_dev, idx_dev, off_dev,
                           fm_dev, fmd_dev);
        if (hipGetLastError() != hipSuccess ||
            (total_matches && hipMemcpyAsync(feature_match_out, fm_dev, (size_t)total_matches * sizeof(edge_feature_match),
                                             hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (total_inliers && hipMemcpyAsync(inlier_match_out, fmd_dev, (size_t)total_inliers * sizeof(edge_inlier_match),
                                             hipMemcpyDeviceToHost, st) != hipSuccess))
            rc = ochip_fail(ctx, OCHIP_EHIP, "edge lists: launch or download failed");
    }
    const hipError_t werr = ochip_stream_wait(ctx, st);
    mem.release();
    if (rc == OCHIP_OK && werr != hipSuccess)
        rc = ochip_fail(ctx, OCHIP_EHIP, "edge lists: %s", hipGetErrorString(werr));
    return rc;
}

int ochip_refit_homography_batch(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, const ochip_ransac_match *matches,
                                 uint64_t total_matches, uint32_t rounds, double inlier_threshold, ochip_ransac_result *results,
                                 uint8_t *inliers)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (n_jobs == 0)
        return OCHIP_OK;
    if (!jobs || !results || rounds == 0 || (total_matches && (!matches || !inliers)))
        return ochip_fail(ctx, OCHIP_EINVAL, "NULL argument or zero rounds");
    if (!ctx->kp_store_ready)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_upload_keypoints has not been called");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    OCHIP_TRY(prepare_homography_jobs(ctx, jobs, n_jobs, total_matches, nullptr));
    const uint64_t T = total_matches ? total_matches : 1;
    ochip::ransac_scratch &rs = ctx->ransac;
    OCHIP_TRY(rs.ensure(ctx, ochip::ransac_writer::refit, n_jobs, sizeof(ochip_ransac_job), T, sizeof(ochip_ransac_match), 0, 0));
    const ochip::ransac_scratch::outputs out = rs.outputs_of(n_jobs);
    OCHIP_HIP(ctx, hipMemcpyAsync(rs.jobs, jobs, (size_t)n_jobs * sizeof(ochip_ransac_job), hipMemcpyHostToDevice, ctx->stream));
    if (total_matches)
    {
        OCHIP_HIP(ctx, hipMemcpyAsync(rs.corr, matches, (size_t)total_matches * sizeof(ochip_ransac_match), hipMemcpyHostToDevice,
                                      ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(out.inliers, inliers, (size_t)total_matches, hipMemcpyHostToDevice, ctx->stream));
    }
    rays_view rv{ctx->rays_dev, ctx->img_off_dev};
    hipLaunchKernelGGL(refit_homography_kernel, dim3(n_jobs), dim3(W), 0, ctx->stream, rs.jobs.as<ochip_ransac_job>(),
                       rs.corr.as<ochip_ransac_match>(), rv, rs.coords, rs.lu, (uint64_t)T, inlier_threshold, rounds, out.results, out.inliers);
    OCHIP_HIP(ctx, hipGetLastError());
    OCHIP_HIP(ctx, hipMemcpyAsync(results, out.results, (size_t)n_jobs * sizeof(ochip_ransac_result), hipMemcpyDeviceToHost, ctx->stream));
    if (total_matches)
        OCHIP_HIP(ctx, hipMemcpyAsync(inliers, out.inliers, (size_t)total_matches, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    return OCHIP_OK;
}


int ochip_debug_homography_fit4(ochip_ctx *ctx, int route, const double *xy16, uint32_t n, double *H9, double *Hinv9,
                                uint8_t *degenerate)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (route != 0 && route != 1)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_homography_fit4: route %d", route);
    if (n == 0)
        return OCHIP_OK;
    if (!xy16 || !H9 || !Hinv9 || !degenerate)
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_homography_fit4: NULL argument");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: the samples (16 doubles each), H and H^-1 (9 each), the degeneracy flags
    const size_t in_bytes = (size_t)n * 16 * 8, m_bytes = (size_t)n * 9 * 8;
    ochip::dev_scratch mem{ctx, "ochip_debug_homography_fit4"};
    double *xy_dev = (double *)mem.get(in_bytes + 2 * m_bytes + n);
    if (!xy_dev)
        return OCHIP_ENOMEM;
    double *H_dev = xy_dev + (size_t)n * 16, *Hi_dev = H_dev + (size_t)n * 9;
    uint8_t *deg_dev = (uint8_t *)(Hi_dev + (size_t)n * 9);
    OCHIP_HIP(ctx, hipMemcpyAsync(xy_dev, xy16, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (route == 0)
        hipLaunchKernelGGL(debug_fit4_kernel<0>, dim3(n), dim3(W), 0, ctx->stream, (const double *)xy_dev, n, H_dev, Hi_dev, deg_dev);
    else
        hipLaunchKernelGGL(debug_fit4_kernel<1>, dim3((n + FB - 1) / FB), dim3(W), 0, ctx->stream, (const double *)xy_dev, n, H_dev,
                           Hi_dev, deg_dev);
    OCHIP_HIP(ctx, hipGetLastError());
    OCHIP_HIP(ctx, hipMemcpyAsync(H9, H_dev, m_bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, hipMemcpyAsync(Hinv9, Hi_dev, m_bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, hipMemcpyAsync(degenerate, deg_dev, n, hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    mem.release();
    return OCHIP_OK;
}

int ochip_debug_decompose_votes(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, const ochip_ransac_match *matches,
                                uint64_t total_matches, const double *H9, const uint8_t *inliers, ochip_decomposition *decomp_out)
{
    if (!ctx)
        return OCHIP_EINVAL;
    if (n_jobs == 0)
        return OCHIP_OK;
    if (!jobs || !H9 || !decomp_out || (total_matches && (!matches || !inliers)))
        return ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_decompose_votes: NULL argument");
    if (!ctx->kp_store_ready)
        return ochip_fail(ctx, OCHIP_ESTATE, "ochip_upload_keypoints has not been called");
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    OCHIP_TRY(prepare_homography_jobs(ctx, jobs, n_jobs, total_matches, nullptr));
    // (the kernel gathers the rays through k1 / k2: a keypoint index past its image would read past the rays)
    for (uint32_t j = 0; j < n_jobs; j++)
        for (uint32_t i = 0; i < jobs[j].n; i++)
        {
            const ochip_ransac_match &m = matches[jobs[j].match_offset + i];
            if (m.k1 >= ctx->img_n[jobs[j].image_1] || m.k2 >= ctx->img_n[jobs[j].image_2])
                return ochip_fail(ctx, OCHIP_EINVAL, "ochip_debug_decompose_votes: job %u, match %u: keypoint index past its image", j, i);
        }
    // result rows that hold nothing but H, as the RANSAC kernel would have left them for the vote
    std::vector<ochip_ransac_result> rows(n_jobs);
    std::memset(rows.data(), 0, (size_t)n_jobs * sizeof(ochip_ransac_result));
    for (uint32_t j = 0; j < n_jobs; j++)
        std::memcpy(rows[j].H, H9 + (size_t)j * 9, sizeof rows[j].H);
    const uint64_t T = total_matches ? total_matches : 1;
    ochip::dev_scratch mem{ctx, "ochip_debug_decompose_votes"};
    ochip_ransac_job *jobs_dev = (ochip_ransac_job *)mem.get((size_t)n_jobs * sizeof(ochip_ransac_job));
    ochip_ransac_match *matches_dev = (ochip_ransac_match *)mem.get((size_t)T * sizeof(ochip_ransac_match));
    ochip_ransac_result *res_dev = (ochip_ransac_result *)mem.get((size_t)n_jobs * sizeof(ochip_ransac_result));
    uint8_t *inl_dev = (uint8_t *)mem.get((size_t)T);
    ochip_decomposition *dec_dev = (ochip_decomposition *)mem.get((size_t)n_jobs * sizeof(ochip_decomposition));
    if (!jobs_dev || !matches_dev || !res_dev || !inl_dev || !dec_dev)
        return OCHIP_ENOMEM;
    OCHIP_HIP(ctx, hipMemcpyAsync(jobs_dev, jobs, (size_t)n_jobs * sizeof(ochip_ransac_job), hipMemcpyHostToDevice, ctx->stream));
    OCHIP_HIP(ctx, hipMemcpyAsync(res_dev, rows.data(), (size_t)n_jobs * sizeof(ochip_ransac_result), hipMemcpyHostToDevice, ctx->stream));
    if (total_matches)
    {
        OCHIP_HIP(ctx, hipMemcpyAsync(matches_dev, matches, (size_t)total_matches * sizeof(ochip_ransac_match), hipMemcpyHostToDevice,
                                      ctx->stream));
        OCHIP_HIP(ctx, hipMemcpyAsync(inl_dev, inliers, (size_t)total_matches, hipMemcpyHostToDevice, ctx->stream));
    }
    rays_view rv{ctx->rays_dev, ctx->img_off_dev};
    hipLaunchKernelGGL(decompose_vote_kernel, dim3((n_jobs + 3) / 4), dim3(256), 0, ctx->stream, (const ochip_ransac_job *)jobs_dev, n_jobs,
                       (const ochip_ransac_match *)matches_dev, (const ochip_ransac_result *)res_dev, (const uint8_t *)inl_dev, rv, dec_dev);
    OCHIP_HIP(ctx, hipGetLastError());
    OCHIP_HIP(ctx, hipMemcpyAsync(decomp_out, dec_dev, (size_t)n_jobs * sizeof(ochip_decomposition), hipMemcpyDeviceToHost, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    mem.release();
    return OCHIP_OK;
}

} // extern "C"
