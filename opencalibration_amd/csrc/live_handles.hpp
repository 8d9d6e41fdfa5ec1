// The registry behind "a destroyed handle is refused, not followed" (std only: shared by libochip.so and liboc_host.so).
#pragma once

#include <mutex>
#include <set>

namespace ochip
{
// The objects of one type that exist.  A destroyed or foreign handle is refused, not followed.  One namespace-scope
// live_set<T> per object type and library: create adds the object last, once it is fully built; every entry asks has();
// destroy goes on (waits, releases, deletes) only where remove() answered true.
template <class T> class live_set
{
  public:
    live_set() = default;
    live_set(const live_set &) = delete;
    live_set &operator=(const live_set &) = delete;

    void add(const T *p)
    {
        std::lock_guard<std::mutex> lock(mutex);
        set.insert(p);
    }
    bool has(const T *p) // false for nullptr
    {
        std::lock_guard<std::mutex> lock(mutex);
        return p && set.count(p) != 0;
    }
    bool remove(const T *p) // true exactly once per add: the caller then frees
    {
        std::lock_guard<std::mutex> lock(mutex);
        return p && set.erase(p) != 0;
    }

  private:
    std::mutex mutex;
    std::set<const T *> set;
};
} // namespace ochip
