// libochip.so: the colour-balance solve on the device (solveColorBalance, src/ortho/color_balance.cpp) as an lm_model
// engine: it owns the radiometric parameters, evaluates cost / J'J / J'r of the colour correspondences into the
// system's tiles, and lm_solve (relax_lm.hip) does everything after the evaluation - build with damping, tile Cholesky,
// back-solve, step control.  The per-correspondence arithmetic is color_balance.hpp's, shared with the CPU route; the plan
// of a solve and the arithmetic of every kernel are color_balance_plan.hpp's, which the host can run as well.
//
// Set-up, once per solve (host): camera and model ids -> table rows, appearance counts (the priors' weights),
// correspondences grouped by (camera pair, model pair) with the side of `a` kept, groups cut into chunks of CHUNK
// correspondences; cameras ordered by reverse Cuthill-McKee over the pair graph and dissected into regions where that
// shortens the factorisation's chain of diagonal tiles (the plane engine's rules, relax.hip: assign_tangent), six
// unknowns per camera, the models' unknowns (and the separator cameras) as the dense tail.
//
// Evaluation, every LM iteration (the Huber weights depend on the residuals: every correspondence is walked):
//   cb_chunk_kernel   one workgroup per chunk.  Lanes own correspondences: corrected Jacobian (3 x 18) and residuals
//                     into LDS.  Then threads own the entries of the chunk's record - the 18 x 18 lower triangle, 18
//                     gradient entries, the cost - and sum them over the chunk's correspondences in index order.
//   cb_gather_kernel  one workgroup per owner of system entries (a camera's diagonal block, a camera pair's block, a
//                     model x camera block, a model's block, a model pair's block): four slices walk the owner's
//                     records in a fixed interleaved order, the slices are added in order, the priors are added, and
//                     the entries are ASSIGNED.  No floating-point atomics anywhere: reruns are bit-identical.
//   cb_segment_kernel an owner of more than 256 records (a model's block: every chunk of a one-model survey) is summed
//                     in two levels: its records 256 at a time here, these partial sums by cb_gather_kernel.
//   cb_cost_kernel    the candidate's evaluation: the cost part of cb_chunk_kernel alone.
//   cb_finish_kernel  total cost (chunks in a fixed tree, priors), and the mail to the host block (lm_mail_post).
#include "color_balance_plan.hpp"
#include "relax_lm.hpp"

#include <cmath>
#include <cstring>

namespace
{
using namespace ochip;
namespace cb = ochip_cb;
using cb::cb_chunk;
using cb::cb_obs;
using cb::cb_owner;

static_assert(cb::NB == LM_NB, "the plan's tile size is the system's");
static_assert(cb::FINISH_WIDTH == LM_TG, "plan_evaluate_host folds the finishing sums as cb_finish_kernel does");
static_assert(cb::REC_ENTRIES <= 256 && cb::GATHER_SLICES * 64 == 256, "thread layout of the chunk and gather kernels");

struct cb_dev
{
    const cb_obs *obs;
    const cb_chunk *chunks;
    uint32_t n_chunks;
    double *x[2];         // current, candidate
    const double *weight; // per unknown: the prior's weight
    double *rec, *chunk_cost;
    double *partial; // [segment][64]: the partial sums of the large owners
    int32_t *fail;
    int n;
};

__global__ __launch_bounds__(256) void cb_chunk_kernel(cb_dev D, int which)
{
    __shared__ double rows[cb::CHUNK * cb::JROW];
    __shared__ double costs[cb::CHUNK];
    const cb_chunk c = D.chunks[blockIdx.x];
    const int t = threadIdx.x;
    if (t < (int)c.count)
    {
        double res[3], cost;
        double *r = rows + t * cb::JROW; // (the Jacobian is formed in place: no private array, no scratch)
        if (!cb::chunk_eval(D.obs, c, (uint32_t)t, D.x[which], res, r, &cost))
            *D.fail = 1;
        r[3 * cb::BLOCK_COLS] = res[0], r[3 * cb::BLOCK_COLS + 1] = res[1], r[3 * cb::BLOCK_COLS + 2] = res[2];
        costs[t] = cost;
    }
    __syncthreads();
    if (t >= cb::REC_ENTRIES)
        return;
    const double s = cb::record_entry(rows, costs, c.count, t);
    if (t == cb::REC_COST)
        D.chunk_cost[blockIdx.x] = s;
    D.rec[(size_t)blockIdx.x * cb::REC + t] = s;
}

// cost only: four chunks per workgroup, a wave each; the chunk's sum in the order cb_chunk_kernel uses
__global__ __launch_bounds__(256) void cb_cost_kernel(cb_dev D, int which)
{
    __shared__ double costs[4 * cb::CHUNK];
    const uint32_t chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    cb_chunk c{};
    if (chunk < D.n_chunks)
        c = D.chunks[chunk];
    if (lane < (int)c.count)
    {
        double res[3], cost;
        if (!cb::chunk_eval(D.obs, c, (uint32_t)lane, D.x[which], res, nullptr, &cost))
            *D.fail = 1;
        costs[threadIdx.x] = cost;
    }
    __syncthreads();
    if (lane == 0 && chunk < D.n_chunks)
        D.chunk_cost[chunk] = cb::record_entry(nullptr, costs + (threadIdx.x & ~63), c.count, cb::REC_COST);
}

// a large owner's records, SEGMENT at a time: one workgroup per segment, summed as cb_gather_kernel sums an owner
__global__ __launch_bounds__(256) void cb_segment_kernel(cb_dev D, const cb::cb_segment *segments, const uint32_t *items)
{
    __shared__ double part[64][cb::GATHER_SLICES];
    const cb::cb_segment sg = segments[blockIdx.x];
    const int e = threadIdx.x & 63, slice = threadIdx.x >> 6, ne = cb::owner_entries(sg.type);
    part[e][slice] = e < ne ? cb::items_slice(D.rec, items, sg.type, sg.swap, sg.first, sg.count, e, slice) : 0.0;
    __syncthreads();
    if (slice == 0)
        D.partial[(size_t)blockIdx.x * 64 + e] = cb::fold_slices(part[e]);
}

__global__ __launch_bounds__(256) void cb_gather_kernel(cb_dev D, const cb_owner *owners, const uint32_t *items, int which, lm_matrix A,
                                                        double *g)
{
    __shared__ double part[64][cb::GATHER_SLICES];
    const cb_owner o = owners[blockIdx.x];
    const int e = threadIdx.x & 63, slice = threadIdx.x >> 6, ne = cb::owner_entries(o.type);
    part[e][slice] = e < ne ? cb::gather_slice(D.rec, items, D.partial, o, e, slice) : 0.0;
    __syncthreads();
    if (slice != 0 || e >= ne)
        return;
    int row = 0, col = 0;
    bool is_g = false;
    const double v = cb::gather_value(part[e], o, e, D.weight, D.x[which], &row, &col, &is_g);
    if (is_g)
        g[row] = v;
    else
        A.tiles[lm_at(A, row, col)] = v;
}

// LM_TG strided partial sums folded by a binary tree (cb::tree_fold is the same sum on the host)
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = LM_TG / 2; s > 0; s >>= 1)
    {
        if (t < s)
            sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(LM_TG) void cb_finish_kernel(cb_dev D, int which, double *scal, lm_mail mail)
{
    __shared__ double sh[LM_TG];
    const int t = threadIdx.x;
    double a = 0, b = 0;
    for (uint32_t k = t; k < D.n_chunks; k += LM_TG)
        a += D.chunk_cost[k];
    for (int i = t; i < D.n; i += LM_TG)
    {
        const double r = D.weight[i] * D.x[which][i];
        b += 0.5 * (r * r);
    }
    const double matches = block_sum(a, sh), priors = block_sum(b, sh);
    if (t == 0)
    {
        scal[0] = matches + priors;
        lm_mail_post(mail);
    }
}

__global__ __launch_bounds__(LM_TG) void cb_candidate_kernel(cb_dev D, const double *y, const double *scale, double alpha, double *scal)
{
    __shared__ double sh[LM_TG];
    const int t = threadIdx.x;
    double step = 0, cand = 0;
    for (int i = t; i < D.n; i += LM_TG)
    {
        const double x = D.x[0][i], c = x + alpha * (-y[i] * scale[i]);
        D.x[1][i] = c;
        step += (x - c) * (x - c);
        cand += c * c;
    }
    const double s2 = block_sum(step, sh), c2 = block_sum(cand, sh);
    if (t == 0)
        scal[2] = s2, scal[3] = c2;
}

struct cb_problem
{
    ochip_ctx *ctx = nullptr;
    dev_blocks mem;
    lm_system sys;
    cb_dev dev{};
    cb_owner *owners_dev = nullptr;
    uint32_t *items_dev = nullptr;
    cb::cb_segment *segments_dev = nullptr;
    uint32_t n_segments = 0;
    uint32_t n_owners = 0, n_cams = 0, n_models = 0;
    uint64_t n_corr = 0;
    std::vector<int32_t> cam_t, model_t;
    ~cb_problem()
    {
        if (!ctx)
            return;
        (void)hipSetDevice(ctx->device);
        (void)ochip_stream_wait(ctx, ctx->stream);
        mem.release();
    }
};

constexpr auto BLOCKING = copy_mode::blocking;

int problem_create(ochip_ctx *ctx, const ochip_color_corr *corr, uint64_t n_corr, const uint64_t *cam_ids, uint32_t n_cams,
                   const uint32_t *model_ids, uint32_t n_models, cb_problem *p)
{
    cb::plan P;
    std::string err;
    if (!cb::build_plan(corr, n_corr, cam_ids, n_cams, model_ids, n_models, &P, &err))
        return ochip_fail(ctx, OCHIP_EINVAL, "%s", err.c_str());
    p->ctx = p->mem.ctx = ctx;
    p->mem.what = "colour balance problem";
    p->n_cams = n_cams, p->n_models = n_models, p->n_corr = n_corr;
    p->cam_t = P.cam_t, p->model_t = P.model_t;
    const int n = P.n;
    lm_envelope env;
    env.env_end = P.env_end, env.first_col = P.first_col, env.region_begin = P.region_begin, env.tail_begin = P.tail_begin;
    if (ochip_verbose("relax"))
        fprintf(stderr, "[ochip colour balance] n=%d cameras=%u models=%u chunks=%zu owners=%zu tail_begin=%d regions=%zu separators=%d\n", n,
                n_cams, n_models, P.chunks.size(), P.owners.size(), P.tail_begin, std::max<size_t>(P.region_begin.size(), 1), P.n_separators);
    const std::vector<cb_obs> &obs = P.obs;
    const std::vector<cb_chunk> &chunks = P.chunks;
    const std::vector<cb_owner> &owners = P.owners;
    const std::vector<uint32_t> &items = P.items;
    const std::vector<double> &weight = P.weight;
    // ---- device side
    OCHIP_HIP(ctx, hipSetDevice(ctx->device));
    cb_dev &D = p->dev;
    int rc = OCHIP_OK;
    auto chk = [&](int r) {
        if (rc == OCHIP_OK)
            rc = r;
    };
    cb_obs *obs_dev = nullptr;
    cb_chunk *chunks_dev = nullptr;
    double *weight_dev = nullptr;
    chk(p->mem.upload(&obs_dev, obs, BLOCKING));
    chk(p->mem.upload(&chunks_dev, chunks, BLOCKING));
    chk(p->mem.upload(&weight_dev, weight, BLOCKING));
    chk(p->mem.upload(&p->owners_dev, owners, BLOCKING));
    chk(p->mem.upload(&p->items_dev, items, BLOCKING));
    chk(p->mem.upload(&p->segments_dev, P.segments, BLOCKING));
    chk(p->mem.alloc<double>(&D.partial, P.segments.size() * 64));
    p->n_segments = (uint32_t)P.segments.size();
    chk(p->mem.alloc<double>(&D.x[0], (size_t)n));
    chk(p->mem.alloc<double>(&D.x[1], (size_t)n));
    chk(p->mem.alloc<double>(&D.rec, chunks.size() * cb::REC));
    chk(p->mem.alloc<double>(&D.chunk_cost, chunks.size()));
    chk(p->mem.alloc<int32_t>(&D.fail, 1));
    if (rc != OCHIP_OK)
        return rc;
    D.obs = obs_dev, D.chunks = chunks_dev, D.weight = weight_dev;
    D.n_chunks = (uint32_t)chunks.size();
    D.n = n;
    p->n_owners = (uint32_t)owners.size();
    // (on the context's stream: the device's default stream is a queue shared with every other context)
    OCHIP_HIP(ctx, hipMemsetAsync(D.x[0], 0, (size_t)n * 8, ctx->stream));
    OCHIP_HIP(ctx, hipMemsetAsync(D.x[1], 0, (size_t)n * 8, ctx->stream));
    OCHIP_HIP(ctx, hipMemsetAsync(D.fail, 0, 4, ctx->stream));
    OCHIP_HIP(ctx, ochip_stream_wait(ctx, ctx->stream));
    p->sys.ctx = ctx;
    p->sys.allocs = &p->mem;
    return lm_system_resize(&p->sys, n, env);
}

struct color_model final : lm_model
{
    cb_problem *p;
    explicit color_model(cb_problem *prob) : p(prob)
    {
    }
    bool mails_results() override
    {
        return true;
    }
    int evaluate(bool with_jac, int which, double *cost) override
    {
        ochip_ctx *ctx = p->ctx;
        hipStream_t st = ctx->stream;
        lm_system &S = p->sys;
        const cb_dev &D = p->dev;
        hipEvent_t e0, e1;
        ochip_prof_begin(ctx, OCHIP_K_RELAX_EVAL, &e0, &e1);
        if (with_jac)
        {
            // the gather ASSIGNS the same entries of A and g at every evaluation; what it leaves alone (fill-in
            // positions) is cleared once per layout
            if (!S.A_clean)
            {
                OCHIP_HIP(ctx, hipMemsetAsync(S.A, 0, S.matrix_bytes(), st));
                OCHIP_HIP(ctx, hipMemsetAsync(S.g, 0, (size_t)S.n * 8, st));
                S.A_clean = true;
            }
            hipLaunchKernelGGL(cb_chunk_kernel, dim3(D.n_chunks), dim3(256), 0, st, D, which);
            if (p->n_segments)
                hipLaunchKernelGGL(cb_segment_kernel, dim3(p->n_segments), dim3(256), 0, st, D, (const cb::cb_segment *)p->segments_dev,
                                   (const uint32_t *)p->items_dev);
            hipLaunchKernelGGL(cb_gather_kernel, dim3(p->n_owners), dim3(256), 0, st, D, (const cb_owner *)p->owners_dev,
                               (const uint32_t *)p->items_dev, which, S.matA(), S.g);
        }
        else
            hipLaunchKernelGGL(cb_cost_kernel, dim3((D.n_chunks + 3) / 4), dim3(256), 0, st, D, which);
        // (the flag is cleared again by the kernel that posts it: no memset in front of the next evaluation)
        const lm_mail mail{S.box, S.scal, S.fail_chol, D.fail, 1, 1, D.fail};
        hipLaunchKernelGGL(cb_finish_kernel, dim3(1), dim3(LM_TG), 0, st, D, which, S.scal, mail);
        ochip_prof_end(ctx, OCHIP_K_RELAX_EVAL, e0, e1);
        OCHIP_HIP(ctx, hipGetLastError());
        if (before_wait)
            before_wait();
        OCHIP_HIP(ctx, ochip_stream_wait(ctx, st));
        *cost = S.box[lm_system::BOX_COST];
        return reinterpret_cast<const int32_t *>(S.box + lm_system::BOX_FAILS)[0] ? 1 : 0;
    }
    void launch_candidate(const double *y, const double *scale, double alpha, double *scal) override
    {
        hipLaunchKernelGGL(cb_candidate_kernel, dim3(1), dim3(LM_TG), 0, p->ctx->stream, p->dev, y, scale, alpha, scal);
    }
    void launch_accept() override
    {
        (void)hipMemcpyAsync(p->dev.x[0], p->dev.x[1], (size_t)p->dev.n * 8, hipMemcpyDeviceToDevice, p->ctx->stream);
    }
    void launch_normalize() override
    {
    }
    int x_norm(double *out) override
    {
        std::vector<double> x((size_t)p->dev.n);
        OCHIP_HIP(p->ctx, hipMemcpy(x.data(), p->dev.x[0], x.size() * 8, hipMemcpyDeviceToHost));
        double s = 0;
        for (double v : x)
            s += v * v;
        *out = std::sqrt(s);
        return OCHIP_OK;
    }
    int num_residual_blocks() override
    {
        return (int)(p->n_corr + 3 * (uint64_t)p->n_cams + p->n_models);
    }
};

int set_state(cb_problem *p, const double *cam6, const double *vig3)
{
    std::vector<double> x((size_t)p->dev.n, 0.0);
    for (uint32_t c = 0; c < p->n_cams; c++)
        std::memcpy(&x[p->cam_t[c]], cam6 + (size_t)cb::CAM_UNKNOWNS * c, sizeof(double) * cb::CAM_UNKNOWNS);
    for (uint32_t m = 0; m < p->n_models; m++)
        std::memcpy(&x[p->model_t[m]], vig3 + (size_t)cb::MODEL_UNKNOWNS * m, sizeof(double) * cb::MODEL_UNKNOWNS);
    OCHIP_HIP(p->ctx, hipMemcpy(p->dev.x[0], x.data(), x.size() * 8, hipMemcpyHostToDevice));
    return OCHIP_OK;
}

int get_state(cb_problem *p, double *cam6, double *vig3)
{
    std::vector<double> x((size_t)p->dev.n);
    OCHIP_HIP(p->ctx, ochip_stream_wait(p->ctx, p->ctx->stream));
    OCHIP_HIP(p->ctx, hipMemcpy(x.data(), p->dev.x[0], x.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < p->n_cams; c++)
        std::memcpy(cam6 + (size_t)cb::CAM_UNKNOWNS * c, &x[p->cam_t[c]], sizeof(double) * cb::CAM_UNKNOWNS);
    for (uint32_t m = 0; m < p->n_models; m++)
        std::memcpy(vig3 + (size_t)cb::MODEL_UNKNOWNS * m, &x[p->model_t[m]], sizeof(double) * cb::MODEL_UNKNOWNS);
    return OCHIP_OK;
}

} // namespace

extern "C"
{

int ochip_color_balance_solve(ochip_ctx *ctx, const ochip_color_corr *corr, uint64_t n_corr, const uint64_t *cam_ids, uint32_t n_cams,
                              const uint32_t *model_ids, uint32_t n_models, double *cam6_out, double *vig3_out,
                              ochip_relax_summary *summary)
{
    if (!ctx || !cam6_out || !vig3_out || !summary)
        return OCHIP_EINVAL;
    *summary = ochip_relax_summary{};
    cb_problem p;
    int rc = problem_create(ctx, corr, n_corr, cam_ids, n_cams, model_ids, n_models, &p);
    if (rc != OCHIP_OK)
        return rc;
    color_model model(&p);
    summary->num_parameters = p.dev.n;
    summary->num_residual_blocks = model.num_residual_blocks();
    ochip_relax_options opt{};
    opt.max_num_iterations = cb::MAX_ITERATIONS;
    opt.initial_trust_region_radius = cb::INITIAL_RADIUS;
    opt.function_tolerance = cb::FUNCTION_TOLERANCE;
    opt.gradient_tolerance = cb::GRADIENT_TOLERANCE;
    opt.parameter_tolerance = cb::PARAMETER_TOLERANCE;
    rc = lm_solve(p.sys, model, &opt, summary);
    if (rc != OCHIP_OK)
        return rc;
    return get_state(&p, cam6_out, vig3_out);
}

int ochip_color_balance_evaluate(ochip_ctx *ctx, const ochip_color_corr *corr, uint64_t n_corr, const uint64_t *cam_ids,
                                 uint32_t n_cams, const uint32_t *model_ids, uint32_t n_models, const double *cam6, const double *vig3,
                                 double *cost, int32_t *n_out, double *JtJ, double *Jtr, int32_t *cam_col, int32_t *model_col)
{
    if (!ctx || !cam6 || !vig3 || !cost)
        return OCHIP_EINVAL;
    cb_problem p;
    int rc = problem_create(ctx, corr, n_corr, cam_ids, n_cams, model_ids, n_models, &p);
    if (rc != OCHIP_OK)
        return rc;
    rc = set_state(&p, cam6, vig3);
    if (rc != OCHIP_OK)
        return rc;
    const int n = p.dev.n;
    if (n_out)
        *n_out = n;
    for (uint32_t c = 0; cam_col && c < n_cams; c++)
        cam_col[c] = p.cam_t[c];
    for (uint32_t m = 0; model_col && m < n_models; m++)
        model_col[m] = p.model_t[m];
    color_model model(&p);
    rc = model.evaluate(JtJ != nullptr || Jtr != nullptr, 0, cost);
    if (rc < 0)
        return rc;
    if (JtJ)
    {
        const int drc = lm_download_dense(p.sys, JtJ);
        if (drc)
            return drc;
    }
    if (Jtr)
        OCHIP_HIP(ctx, hipMemcpy(Jtr, p.sys.g, (size_t)n * 8, hipMemcpyDeviceToHost));
    return rc;
}

} // extern "C"