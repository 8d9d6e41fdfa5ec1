// Driver of tests/test_extract_slots.py: surveys as threads on one extract_slots object, following the protocol of
// extract_features_stream (host/extract_features.cpp) with sleeps in place of the device and the host tail.
//   extract_slots_driver random SEED N   N seeded random schedules: 2 - 4 surveys x 1 - 13 chunks x 1 - 5 slots, random
//                                        chunk durations, one survey failing half-way
//   extract_slots_driver handover        two surveys of 10 equal chunks on 4 slots: survey 1 must be running on a slot
//                                        that survey 0 freed before survey 0's last chunk has finished
// Exit status 0 and a last line "ok ..." when every invariant held; a line "FAIL ..." and status 1 otherwise.
#include "../opencalibration_amd/csrc/host/extract_slots.hpp"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <string>
#include <thread>
#include <vector>

using namespace opencalibration_amd;
using clk = std::chrono::steady_clock;

static std::atomic<int> g_failures{0};
static void fail(const char *what, long a = 0, long b = 0)
{
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    g_failures++;
}

struct world
{
    extract_slots slots;
    std::atomic<int> holders[extract_slots::MAX_SLOTS];
    std::atomic<int> users[extract_slots::MAX_SLOTS][extract_slots::BUFFERS_PER_SLOT];
    std::atomic<int> in_flight{0};
    std::mutex log_mu;
    struct handed
    {
        uint64_t ticket;
        uint32_t chunk, slot;
        clk::time_point start, end;
    };
    std::vector<handed> log; // in hand-out order
    world()
    {
        for (auto &h : holders)
            h = 0;
        for (auto &s : users)
            for (auto &u : s)
                u = 0;
    }
};

struct survey_plan
{
    uint32_t chunks, drivers;
    std::vector<int> chunk_us;
    int tail_us;
    int fail_at; // chunk that fails (-1: none)
    extract_slots::order how;
};

// what extract_features_stream does with the slots; returns false if the survey failed
static bool run_survey(world &w, const survey_plan &p, uint64_t *ticket_out)
{
    const uint32_t n_drivers = std::min(p.drivers, p.chunks);
    extract_ticket ticket(w.slots, n_drivers);
    *ticket_out = ticket.id();
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<uint32_t, int>> ready;
    uint32_t next_chunk = 0, drivers_done = 0;
    bool failed = false;
    auto driver = [&](uint32_t d) {
        {
            slot_hold hold(w.slots, ticket.id(), d, p.how);
            if (w.holders[d].fetch_add(1) != 0)
                fail("two holders of a slot", d);
            for (;;)
            {
                uint32_t c = 0;
                bool go = false;
                size_t entry = 0;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (!failed && next_chunk < p.chunks)
                    {
                        c = next_chunk++;
                        go = true;
                        std::lock_guard<std::mutex> lg(w.log_mu);
                        entry = w.log.size();
                        w.log.push_back({ticket.id(), c, d, clk::now(), clk::time_point::max()});
                    }
                }
                if (!go)
                    break;
                if (c + 1 == p.chunks && p.how == extract_slots::order::slot)
                    ticket.retire();
                const int b = w.slots.take_buffer(d);
                if (w.users[d][b].fetch_add(1) != 0)
                    fail("a buffer handed to two users", d, b);
                extract_slots::buffer &sb = w.slots.at(d, b);
                sb.layout = (int)(ticket.id() & 1); // (the holder may reshape the buffer it took)
                sb.bytes[0] = p.chunks;
                const int now = w.in_flight.fetch_add(1) + 1;
                if (now > (int)w.slots.slots())
                    fail("more chunks in flight than slots", now, w.slots.slots());
                std::this_thread::sleep_for(std::chrono::microseconds(p.chunk_us[c]));
                w.in_flight.fetch_sub(1);
                {
                    std::lock_guard<std::mutex> lg(w.log_mu);
                    w.log[entry].end = clk::now();
                }
                std::unique_lock<std::mutex> lk(mu);
                if ((int)c == p.fail_at)
                {
                    failed = true;
                    lk.unlock();
                    cv.notify_all();
                    w.users[d][b].fetch_sub(1);
                    w.slots.return_buffer(d, b);
                    ticket.retire();
                    break;
                }
                ready.emplace_back(d, b);
                cv.notify_all();
            }
            w.holders[d].fetch_sub(1);
        }
        std::lock_guard<std::mutex> lk(mu);
        drivers_done++;
        cv.notify_all();
    };
    std::vector<std::thread> drivers;
    for (uint32_t d = 0; d < n_drivers; d++)
        drivers.emplace_back(driver, d);
    for (;;)
    {
        std::pair<uint32_t, int> which;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !ready.empty() || drivers_done == n_drivers; });
            if (ready.empty())
                break;
            which = ready.front();
            ready.pop_front();
        }
        std::this_thread::sleep_for(std::chrono::microseconds(p.tail_us)); // the host tail reads the buffer
        const extract_slots::buffer &sb = w.slots.at(which.first, which.second);
        if (sb.layout != (int)(ticket.id() & 1) || sb.bytes[0] != p.chunks)
            fail("a buffer changed under its reader", which.first, which.second);
        w.users[which.first][which.second].fetch_sub(1);
        w.slots.return_buffer(which.first, which.second);
    }
    for (auto &t : drivers)
        t.join();
    ticket.retire();
    return !failed;
}

static void check_order(const world &w, extract_slots::order how)
{
    // chunks are handed out in ticket order, and within a ticket in chunk order
    if (how == extract_slots::order::none)
        return;
    for (size_t i = 1; i < w.log.size(); i++)
    {
        const auto &a = w.log[i - 1], &b = w.log[i];
        if (b.ticket < a.ticket || (b.ticket == a.ticket && b.chunk != a.chunk + 1))
            fail("chunks handed out of ticket order", (long)b.ticket, (long)b.chunk);
    }
}

static int random_schedules(unsigned seed, int n)
{
    std::mt19937 rng(seed);
    auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    long chunks_total = 0;
    for (int s = 0; s < n; s++)
    {
        world w;
        const int n_surveys = uni(2, 4);
        const int mode = uni(0, 9);
        const extract_slots::order how = mode == 0 ? extract_slots::order::survey : mode == 1 ? extract_slots::order::none : extract_slots::order::slot;
        const int failing = uni(0, n_surveys - 1);
        std::vector<survey_plan> plans(n_surveys);
        for (int k = 0; k < n_surveys; k++)
        {
            survey_plan &p = plans[k];
            p.chunks = (uint32_t)uni(1, 13);
            p.drivers = (uint32_t)uni(1, 5);
            for (uint32_t c = 0; c < p.chunks; c++)
                p.chunk_us.push_back(uni(0, 3) == 0 ? uni(500, 3000) : uni(20, 600));
            p.tail_us = uni(10, 800);
            p.fail_at = k == failing ? (int)p.chunks / 2 : -1;
            p.how = how;
            chunks_total += p.chunks;
        }
        std::vector<std::thread> threads;
        std::vector<uint64_t> tickets(n_surveys, 0);
        std::vector<char> ok(n_surveys, 0);
        for (int k = 0; k < n_surveys; k++)
        {
            threads.emplace_back([&, k] { ok[k] = run_survey(w, plans[k], &tickets[k]); });
            if (uni(0, 1))
                std::this_thread::sleep_for(std::chrono::microseconds(uni(0, 400)));
        }
        for (auto &t : threads)
            t.join();
        check_order(w, how);
        for (int k = 0; k < n_surveys; k++)
        {
            if (ok[k] != (k != failing))
                fail("a survey's result is not its plan's", k, ok[k]);
            // a survey that did not fail was handed every chunk
            long mine = 0;
            for (const auto &h : w.log)
                mine += h.ticket == tickets[k];
            if (k != failing && mine != (long)plans[k].chunks)
                fail("a survey missed chunks", k, mine);
        }
        if (w.in_flight.load() != 0)
            fail("chunks left in flight");
        if (g_failures.load())
        {
            std::printf("FAIL schedule %d of seed %u\n", s, seed);
            return 1;
        }
    }
    std::printf("ok %d schedules, %ld chunks\n", n, chunks_total);
    return 0;
}

static int handover_case()
{
    world w;
    survey_plan p;
    p.chunks = 10;
    p.drivers = 4;
    p.chunk_us.assign(10, 30000);
    p.tail_us = 3000;
    p.fail_at = -1;
    p.how = extract_slots::order::slot;
    // (two surveys: the first starts its four sequences together, so its rounds are 4, 4, 2 and two slots fall free a whole
    // chunk before its last chunk ends; a third survey of equal chunks would follow a survey whose sequences are out of
    // step by exactly one round and finish together)
    constexpr int N = 2;
    uint64_t t[N];
    std::vector<std::thread> threads;
    for (int k = 0; k < N; k++)
    {
        threads.emplace_back([&, k] { run_survey(w, p, &t[k]); });
        std::this_thread::sleep_for(std::chrono::milliseconds(5)); // arrival order = k
    }
    for (auto &th : threads)
        th.join();
    check_order(w, p.how);
    for (uint64_t k = 0; k + 1 < (uint64_t)N; k++)
    {
        clk::time_point last_end = clk::time_point::min(), next_start = clk::time_point::max();
        uint32_t next_slot = 0;
        std::vector<char> used_by_k(extract_slots::MAX_SLOTS, 0);
        for (const auto &h : w.log)
        {
            if (h.ticket == k)
            {
                last_end = std::max(last_end, h.end);
                used_by_k[h.slot] = 1;
            }
            if (h.ticket == k + 1 && h.start < next_start)
            {
                next_start = h.start;
                next_slot = h.slot;
            }
        }
        const double lead = std::chrono::duration<double, std::milli>(last_end - next_start).count();
        std::printf("survey %lu -> %lu: survey %lu started on slot %u %.1f ms before survey %lu's last chunk finished\n",
                    (unsigned long)k, (unsigned long)(k + 1), (unsigned long)(k + 1), next_slot, lead, (unsigned long)k);
        if (!(next_start < last_end))
            fail("the next survey did not start before the last chunk of the survey before finished", (long)k);
        if (!used_by_k[next_slot])
            fail("the next survey started on a slot the survey before never used", (long)k, next_slot);
    }
    if (g_failures.load())
        return 1;
    std::printf("ok handover\n");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "random" && argc > 3)
        return random_schedules((unsigned)std::atol(argv[2]), std::atoi(argv[3]));
    if (mode == "handover")
        return handover_case();
    std::fprintf(stderr, "usage: %s random SEED N | handover\n", argv[0]);
    return 2;
}
