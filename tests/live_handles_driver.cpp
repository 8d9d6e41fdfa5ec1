// A stand-alone program over csrc/live_handles.hpp, for the sanitizers (tests/test_live_handles.py builds it with the
// address and undefined-behaviour sanitizers, and once more with the thread sanitizer): the answers of one set, two sets
// of different types over the same addresses, and 8 threads that add, query and remove while a ninth polls.
#include "../opencalibration_amd/csrc/live_handles.hpp"

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

namespace
{
struct apple
{
    int v = 0;
};
struct pear; // never defined: a set takes an opaque type, as the libraries' handles are

ochip::live_set<apple> g_apples; // namespace scope, as in the libraries
ochip::live_set<pear> g_pears;

int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok)
    {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

void one_set()
{
    apple a, b;
    expect(!g_apples.has(nullptr), "has(nullptr) is false");
    expect(!g_apples.remove(nullptr), "remove(nullptr) is false");
    expect(!g_apples.has(&a), "an address never added is refused");
    expect(!g_apples.remove(&a), "an address never added is not removed");
    g_apples.add(&a);
    expect(g_apples.has(&a), "has after add");
    expect(!g_apples.has(&b), "the neighbour was not added");
    expect(g_apples.remove(&a), "the first remove is true");
    expect(!g_apples.remove(&a), "the second remove is false");
    expect(!g_apples.has(&a), "has after remove is false");
}

void two_types()
{
    apple a;
    const pear *same = reinterpret_cast<const pear *>(&a);
    g_apples.add(&a);
    expect(!g_pears.has(same), "a set of another type does not see the address");
    expect(!g_pears.remove(same), "... and does not remove it");
    expect(g_apples.has(&a), "... which stays live in its own set");
    g_pears.add(same);
    expect(g_apples.remove(&a), "removed from its own set");
    expect(g_pears.has(same), "the other set keeps its own entry");
    expect(g_pears.remove(same) && !g_pears.has(same) && !g_apples.has(&a), "both sets are empty again");
}

void threads()
{
    constexpr int THREADS = 8, EACH = 10000;
    std::vector<apple> objects((size_t)THREADS * EACH);
    std::vector<std::atomic<int>> removed(objects.size());
    for (std::atomic<int> &r : removed)
        r.store(0);
    std::atomic<int> wrong{0}, running{THREADS};
    std::atomic<long long> seen{0};
    std::thread poller([&] {
        long long n = 0;
        do
            for (const apple &o : objects)
                n += g_apples.has(&o) ? 1 : 0;
        while (running.load() != 0);
        seen.store(n);
    });
    std::vector<std::thread> workers;
    for (int t = 0; t < THREADS; t++)
        workers.emplace_back([&, t] {
            apple *mine = objects.data() + (size_t)t * EACH;
            for (int i = 0; i < EACH; i++)
                g_apples.add(mine + i);
            for (int i = 0; i < EACH; i++)
                wrong += g_apples.has(mine + i) ? 0 : 1;
            for (int i = 0; i < EACH; i++)
            {
                removed[(size_t)t * EACH + i] += g_apples.remove(mine + i) ? 1 : 0;
                removed[(size_t)t * EACH + i] += g_apples.remove(mine + i) ? 1 : 0;
                wrong += g_apples.has(mine + i) ? 1 : 0;
            }
            running--;
        });
    for (std::thread &w : workers)
        w.join();
    poller.join();
    expect(wrong.load() == 0, "every object was live between its add and its remove, and not after");
    bool once = true, empty = true;
    for (size_t i = 0; i < objects.size(); i++)
    {
        once = once && removed[i].load() == 1;
        empty = empty && !g_apples.has(&objects[i]);
    }
    expect(once, "every remove returned true exactly once");
    expect(empty, "the set is empty at the end");
    std::printf("polled %lld live answers\n", seen.load());
}
} // namespace

int main()
{
    one_set();
    two_types();
    threads();
    if (failures == 0)
        std::printf("ok\n");
    return failures ? 1 : 0;
}
