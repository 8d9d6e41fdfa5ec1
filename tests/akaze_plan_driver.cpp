// AKAZE's plan (csrc/akaze_plan.hpp) walked on the CPU: for seven calls the plan is built and executed symbolically -
// every plane holds a tag, a launch checks the tag of the plane it reads and writes "level i after k steps" - and the
// routes and the per-level table are compared with what the kernels are instantiated for.  Stand-alone: no device
// library, nothing loaded into Python (tests/test_akaze_plan.py builds it with the sanitizers and runs it).
#include "../opencalibration_amd/csrc/akaze_plan.hpp"

#include <cstdio>
#include <string>

using namespace ochip::akaze;

static int failures = 0;
static std::string where;
#define CHECK(cond, ...)                                                                                               \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(cond))                                                                                                   \
        {                                                                                                              \
            failures++;                                                                                                \
            std::printf("FAILED %s: %s: ", where.c_str(), #cond);                                                      \
            std::printf(__VA_ARGS__);                                                                                  \
            std::printf("\n");                                                                                         \
        }                                                                                                              \
    } while (0)

// what a plane holds: level `level` after `steps` of its FED steps (a level's first image: 0 steps), or nothing yet
struct tag
{
    int level = -1, steps = -1;
    bool operator==(const tag &o) const { return level == o.level && steps == o.steps; }
};

struct planes
{
    tag lt[16], ping;
    int flow = -1; // the level whose conductivity the plane holds
    tag &at(const plane_ref &r) { return r.id == plane_id::level ? lt[r.level] : ping; }
};

// the table of the issue: levels 0 .. 15
static const int SIGMA_SIZE[16] = {2, 3, 3, 4, 2, 3, 3, 4, 2, 3, 3, 4, 2, 3, 3, 4};
static const int FED_STEPS[16] = {0, 3, 3, 4, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 24, 29};

struct built
{
    level_table T;
    plan P;
};

static built run_case(const char *name, int W, int H, const plan_inputs &in, int want_octaves)
{
    where = name;
    built b{level_table(W, H), {}};
    b.P = make_plan(b.T, W, H, in);
    const levels_dev &LV = b.T.LV;
    const plan &P = b.P;
    CHECK(P.error == nullptr, "%s", P.error);
    if (P.error)
        return b;
    CHECK(LV.n == 4 * want_octaves, "%d levels", LV.n);
    CHECK((int)P.lv.size() == LV.n, "%zu level plans", P.lv.size());

    planes M;
    M.lt[0] = {0, 0}; // the base image: level 0 has no steps
    CHECK(P.lv[0].launches.empty() && !P.lv[0].strip, "level 0 is the base image");
    for (int i = 0; i < LV.n; i++)
    {
        CHECK(LV.l[i].sigma_size == SIGMA_SIZE[i], "level %d: sigma_size %d", i, LV.l[i].sigma_size);
        CHECK((int)b.T.tsteps[i].size() == FED_STEPS[i], "level %d: %zu steps", i, b.T.tsteps[i].size());
        const det_window_t w = P.lv[i].det_win;
        CHECK(w.x0 > w.x1 || (w.x0 >= 1 && w.x1 <= LV.l[i].w - 2), "level %d: columns %d .. %d", i, w.x0, w.x1);
        CHECK(w.y0 > w.y1 || (w.y0 >= 1 && w.y1 <= LV.l[i].h - 2), "level %d: rows %d .. %d", i, w.y0, w.y1);
    }
    for (int i = 1; i < LV.n; i++)
    {
        where = std::string(name) + " level " + std::to_string(i);
        const level_info &l = LV.l[i], &p = LV.l[i - 1];
        const level_plan &lp = P.lv[i], &pp = P.lv[i - 1];
        const int n_steps = (int)b.T.tsteps[i].size();
        const bool boundary = l.octave > p.octave;
        int sum = 0;
        for (int g : lp.groups)
        {
            CHECK(g >= 1 && g <= FED_FUSE, "a group of %d", g);
            sum += g;
        }
        CHECK(sum == n_steps, "groups sum to %d of %d", sum, n_steps);
        CHECK(lp.half_out.id == plane_id::none || lp.strip, "only a strip launch has the epilogue");

        // the image the level starts from: the previous level's last image, half-sampled at a new octave
        const tag start = boundary ? tag{i, 0} : tag{i - 1, (int)b.T.tsteps[i - 1].size()};
        int done = 0, n_diffuse_or_strip = 0, n_first = 0, n_half = 0;
        for (size_t q = 0; q < lp.launches.size(); q++)
        {
            const launch &L = lp.launches[q];
            CHECK(!(L.src == L.dst), "launch %zu reads and writes the same plane", q);
            CHECK(L.src.id == plane_id::level || L.src.id == plane_id::ping, "launch %zu reads an image plane", q);
            switch (L.kind)
            {
            case launch_kind::halfsample:
            case launch_kind::halfsample_area:
                CHECK(q == 0 && boundary, "a half-sample opens an octave");
                CHECK((L.kind == launch_kind::halfsample_area) == (p.w != 2 * l.w || p.h != 2 * l.h), "the area path is for odd sizes");
                CHECK(pp.half_out.id == plane_id::none, "the epilogue of level %d wrote this image already", i - 1);
                CHECK((L.src == plane_ref{plane_id::level, i - 1}), "reads the level before");
                CHECK((M.at(L.src) == tag{i - 1, (int)b.T.tsteps[i - 1].size()}), "level %d is not finished", i - 1);
                CHECK(L.dst.id == plane_id::ping || (L.dst == plane_ref{plane_id::level, i}), "writes ping or the level plane");
                M.at(L.dst) = {i, 0};
                n_half++;
                break;
            case launch_kind::smooth:
                CHECK(!lp.strip && n_first == 0, "one Lsmooth launch of a tile level");
                CHECK(M.at(L.src) == start, "reads level %d after %d steps", M.at(L.src).level, M.at(L.src).steps);
                CHECK(L.dst.id == plane_id::flow, "writes the conductivity");
                M.flow = i;
                n_first++;
                break;
            case launch_kind::strip:
                CHECK(lp.strip && n_first == 0, "one strip launch of a strip level");
                CHECK(M.at(L.src) == start, "reads level %d after %d steps", M.at(L.src).level, M.at(L.src).steps);
                CHECK(L.first_step == 0 && L.n_steps == lp.groups[0], "carries the first group");
                CHECK(instantiated(l.sigma_size, L.n_steps), "level_strip_kernel<%d, %d, %d>", l.sigma_size, L.n_steps, (int)lp.store_flow);
                CHECK(L.dst.id == plane_id::ping || (L.dst == plane_ref{plane_id::level, i}), "writes ping or the level plane");
                if (lp.store_flow)
                    M.flow = i;
                M.at(L.dst) = {i, L.n_steps};
                done = L.n_steps;
                if (lp.half_out.id != plane_id::none)
                {
                    CHECK(i + 1 < LV.n && LV.l[i + 1].octave > l.octave, "the epilogue closes an octave");
                    CHECK(done == n_steps, "the epilogue halves the level's last image");
                    CHECK(l.w == 2 * LV.l[i + 1].w && l.h == 2 * LV.l[i + 1].h, "the epilogue halves even sizes");
                    CHECK(!(lp.half_out == L.src) && !(lp.half_out == L.dst), "the epilogue writes a third plane");
                    M.at(lp.half_out) = {i + 1, 0};
                }
                n_first++;
                n_diffuse_or_strip++;
                break;
            case launch_kind::diffuse:
                CHECK(n_first == 1, "the diffusion follows the level's first launch");
                CHECK(L.first_step == done && L.n_steps >= 1 && L.n_steps <= FED_FUSE, "steps %d + %d after %d", L.first_step, L.n_steps, done);
                CHECK((M.at(L.src) == (done == 0 ? start : tag{i, done})), "reads level %d after %d steps", M.at(L.src).level, M.at(L.src).steps);
                CHECK(M.flow == i, "the conductivity plane holds level %d's", M.flow);
                CHECK(!lp.strip || lp.store_flow, "a diffusion launch behind a strip launch needs the stored conductivity");
                CHECK(L.dst.id == plane_id::ping || (L.dst == plane_ref{plane_id::level, i}), "writes ping or the level plane");
                M.at(L.dst) = {i, done + L.n_steps};
                done += L.n_steps;
                n_diffuse_or_strip++;
                break;
            }
        }
        CHECK(n_first == 1, "%d first launches", n_first);
        CHECK(n_diffuse_or_strip == (int)lp.groups.size(), "%d launches for %zu groups", n_diffuse_or_strip, lp.groups.size());
        CHECK(n_half == (boundary && pp.half_out.id == plane_id::none ? 1 : 0), "%d half-sample launches", n_half);
        if (boundary && pp.half_out.id != plane_id::none)
            CHECK(lp.launches[0].src == pp.half_out, "the first launch reads what the epilogue wrote");
        CHECK((M.lt[i] == tag{i, n_steps}), "Lt holds level %d after %d steps", M.lt[i].level, M.lt[i].steps);
    }
    where = name;
    return b;
}

// are all levels of octave o (determinant: 0 .. 3; levels: those >= 1) strips?
static bool octave_is(const built &b, int o, bool strips)
{
    bool all = true;
    for (int i = 0; i < b.T.LV.n; i++)
        if (b.T.LV.l[i].octave == o)
            all = all && b.P.lv[i].det_strip == strips && (i == 0 || b.P.lv[i].strip == strips);
    return all;
}

int main()
{
    {
        plan_inputs in;
        in.B = 100;
        const built a = run_case("a (the bench chunk)", 1600, 1200, in, 4);
        CHECK(a.P.contrast_strip && a.P.det_accumulate, "the contrast pass of 192 M pixels takes the strips");
        CHECK(octave_is(a, 0, true) && octave_is(a, 1, true), "192 M and 48 M pixels per launch: strips");
        CHECK(octave_is(a, 2, false) && octave_is(a, 3, false), "12 M and 3 M pixels per launch: tiles");
        // the levels of the first octave run their whole cycle in one launch, the last one with the half-sampling epilogue
        CHECK(!a.P.lv[1].store_flow && !a.P.lv[3].store_flow && a.P.lv[3].half_out.id != plane_id::none, "octave 0 in one launch per level");
        CHECK(a.P.lv[7].store_flow && a.P.lv[7].half_out.id == plane_id::none, "level 7 has two groups");
    }
    {
        plan_inputs in;
        in.strip_min_pixels = 320 * 160;
        const built b = run_case("b (the planes test's mixed route)", 640, 320, in, 4);
        CHECK(!b.P.contrast_strip, "the contrast pass keeps the built-in threshold");
        CHECK(octave_is(b, 0, true) && octave_is(b, 1, true) && octave_is(b, 2, false) && octave_is(b, 3, false), "strips on octaves 0 - 1");
    }
    {
        plan_inputs in;
        in.tile_levels = in.tile_det = true;
        const built c = run_case("c (tile_levels,tile_det)", 640, 480, in, 4);
        CHECK(!c.P.contrast_strip && !c.P.det_accumulate, "no strips");
        for (int o = 0; o < 4; o++)
            CHECK(octave_is(c, o, false), "octave %d", o);
    }
    {
        plan_inputs in;
        in.strip_levels = in.strip_det = true;
        const built d = run_case("d (strip_levels,strip_det)", 640, 480, in, 4);
        CHECK(d.P.contrast_strip && d.P.det_accumulate, "strips");
        for (int i = 0; i < d.T.LV.n; i++)
        {
            const level_info &l = d.T.LV.l[i];
            CHECK(d.P.lv[i].det_strip, "determinant of level %d", i);
            CHECK(d.P.lv[i].strip == (i > 0 && l.w >= 64 && l.h >= 64 && l.w % 2 == 0 && l.h % 2 == 0), "level %d of %d x %d", i, l.w, l.h);
        }
        CHECK(d.P.lv[8].strip && !d.P.lv[12].strip, "160 x 120 in strips, 80 x 60 in tiles");
        plan_inputs dump = in;
        dump.keep_flow = true;
        const built k = run_case("d with the planes kept", 640, 480, dump, 4);
        CHECK(k.P.lv[1].store_flow && !d.P.lv[1].store_flow, "OCHIP_DUMP_PLANES keeps the conductivity plane");
        plan_inputs un = in;
        un.aligned16 = false;
        const built u = run_case("d unaligned", 640, 480, un, 4);
        CHECK(!u.P.contrast_strip && !u.P.det_accumulate && octave_is(u, 0, false), "unaligned planes take the tiles");
    }
    {
        const built e = run_case("e (odd sizes)", 501, 334, plan_inputs{}, 3);
        CHECK(!e.P.contrast_strip && !e.P.det_accumulate, "no strips");
        for (int o = 0; o < 3; o++)
            CHECK(octave_is(e, o, false), "octave %d", o);
        CHECK(e.P.lv[4].launches[0].kind == launch_kind::halfsample_area && e.P.lv[8].launches[0].kind == launch_kind::halfsample_area,
              "501 -> 250 -> 125: the area half-sample at both boundaries");
    }
    {
        const built f = run_case("f (three octaves)", 640, 200, plan_inputs{}, 3);
        CHECK(f.T.LV.l[11].w == 160 && f.T.LV.l[11].h == 50, "the last octave is 160 x 50");
    }
    {
        run_case("g (a single octave)", 72, 48, plan_inputs{}, 1);
    }
    // the whole table, all sixteen levels
    {
        where = "table";
        const level_table T(1600, 1200);
        CHECK(T.LV.n == 16, "%d levels", T.LV.n);
        CHECK(gaussian_taps(1.0f).size() == 5 && gaussian_taps(SIGMA_OFFSET).size() == 9, "Gaussian kernels of 5 and 9 taps");
    }
    if (failures)
    {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
