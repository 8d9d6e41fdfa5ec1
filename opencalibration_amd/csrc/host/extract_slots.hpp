// Hand-over of the extraction contexts from one survey to the next (header-only, plain C++: no device call in here, so
// tests/test_extract_slots.py drives it from a small program of its own under the thread sanitizer).
//
// A root device context extracts with n "slots": slot d is its sibling 21 + d, a context nothing else uses, with a stream of
// the lowest priority (OCHIP_EXTRACT_PRIORITY=0: slot 0 is the context itself, slot d its sibling d - 1).  A context is
// not thread-safe - its stream, device pool, page-locked pool and error string belong to ONE thread at a time - so a
// slot has one holder.  Surveys (calls of extract_features_stream on the same root context, from any threads) take a
// ticket on entry.  Driver d of a survey may start on slot d when the slot is free AND every survey with an earlier
// ticket has handed out its last chunk; a driver that finds no chunk left gives its slot back at once, while the
// survey's other chunks still run, and the survey behind it starts there.  So chunks are issued strictly in ticket
// order, at most n are in flight (one arena of device memory per context, as before), and the device keeps n launch
// sequences across a survey boundary instead of draining to none.
//
// The page-locked result buffers belong to the slot, not to a survey: BUFFERS_PER_SLOT of them, allocated by whoever
// holds the slot when one is missing, too small or of the other layout, and kept for the life of the root context.  The
// holder takes a free buffer for every chunk; the consumer of the survey that filled it (its calling thread, running the
// host tail) gives it back.  Three per slot: one being filled, one in its survey's host tail, and one that a survey that
// has already left the slot may still be reading when the next survey's driver wants to fill its first.
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <set>

namespace opencalibration_amd
{

class extract_slots
{
  public:
    static constexpr uint32_t MAX_SLOTS = 8;
    static constexpr int BUFFERS_PER_SLOT = 3;
    enum class order
    {
        slot,   // the next survey's driver d starts when slot d is free and the surveys before have no chunk left to hand out
        survey, // ... when the surveys before have FINISHED (the whole-extraction gate of rounds 4 to 6)
        none    // no ordering between surveys: a driver only waits for its slot to be free
    };
    struct buffer
    {
        void *block[2] = {nullptr, nullptr}; // page-locked; layout 0: one block (prepared lists), 1: keypoints + descriptors
        size_t bytes[2] = {0, 0};
        int layout = -1;
        bool busy = false;
    };

    // arrival order; the slot count is the largest driver count asked for so far
    uint64_t enter(uint32_t n_drivers)
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (n_drivers > n_slots_)
            n_slots_ = n_drivers < MAX_SLOTS ? n_drivers : MAX_SLOTS;
        return next_ticket_++;
    }
    uint32_t slots() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        return n_slots_;
    }
    // Blocks until driver d of `ticket` may use slot d.
    void acquire(uint64_t ticket, uint32_t d, order how)
    {
        std::unique_lock<std::mutex> lk(mu_);
        // (serving_ > ticket: the survey's own last chunk was handed out before this driver got here - it takes the slot,
        // finds nothing to do and gives it back.  Such a late driver competes for the slot with driver d of the survey behind
        // and, if that one wins, waits for it to run out of chunks: only a survey with about as many chunks as drivers can
        // have one - with 10 chunks on 4 slots every driver has its slot within a chunk's time - and it delays that survey's
        // return, not the device)
        cv_.wait(lk, [&] { return !slot_[d].held && (how == order::none || serving_ >= ticket); });
        slot_[d].held = true;
        slot_[d].holder = ticket;
    }
    void release(uint64_t ticket, uint32_t d)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!slot_[d].held || slot_[d].holder != ticket)
                return;
            slot_[d].held = false;
        }
        cv_.notify_all();
    }
    // The survey has handed out its last chunk (or gives up): the one behind it may start where slots are free.
    // Tickets may retire in any order (a survey that fails before its turn); may be called more than once.
    void retire(uint64_t ticket)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (ticket < serving_ || !retired_.insert(ticket).second)
                return;
            while (!retired_.empty() && *retired_.begin() == serving_)
            {
                retired_.erase(retired_.begin());
                serving_++;
            }
        }
        cv_.notify_all();
    }
    // For the holder of slot d: a buffer nobody fills or reads (waits for one), marked busy.  The holder may replace its
    // blocks before filling it.
    int take_buffer(uint32_t d)
    {
        std::unique_lock<std::mutex> lk(mu_);
        int b = -1;
        cv_.wait(lk, [&] {
            for (int i = 0; i < BUFFERS_PER_SLOT; i++)
                if (!slot_[d].buf[i].busy)
                {
                    b = i;
                    return true;
                }
            return false;
        });
        slot_[d].buf[b].busy = true;
        return b;
    }
    // From any thread: whoever read the buffer is done with it.
    void return_buffer(uint32_t d, int b)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            slot_[d].buf[b].busy = false;
        }
        cv_.notify_all();
    }
    // (only the thread that took the buffer, until it is returned)
    buffer &at(uint32_t d, int b) { return slot_[d].buf[b]; }

  private:
    struct slot
    {
        bool held = false;
        uint64_t holder = 0;
        buffer buf[BUFFERS_PER_SLOT];
    };
    mutable std::mutex mu_;
    std::condition_variable cv_;
    slot slot_[MAX_SLOTS];
    uint32_t n_slots_ = 0;
    uint64_t next_ticket_ = 0, serving_ = 0; // serving_: the oldest ticket that still has chunks to hand out
    std::set<uint64_t> retired_;            // retired ahead of serving_
};

// A survey's stay: the ticket, retired on every return path; the slots its drivers hold are released by them (slot_hold).
class extract_ticket
{
  public:
    extract_ticket(extract_slots &s, uint32_t n_drivers) : slots_(s), ticket_(s.enter(n_drivers)) {}
    ~extract_ticket() { slots_.retire(ticket_); }
    extract_ticket(const extract_ticket &) = delete;
    extract_ticket &operator=(const extract_ticket &) = delete;
    uint64_t id() const { return ticket_; }
    void retire() { slots_.retire(ticket_); }

  private:
    extract_slots &slots_;
    uint64_t ticket_;
};

// A driver's hold of its slot, given back when the driver leaves on whatever path.
class slot_hold
{
  public:
    slot_hold(extract_slots &s, uint64_t ticket, uint32_t d, extract_slots::order how) : slots_(s), ticket_(ticket), d_(d)
    {
        slots_.acquire(ticket_, d_, how);
    }
    ~slot_hold() { slots_.release(ticket_, d_); }
    slot_hold(const slot_hold &) = delete;
    slot_hold &operator=(const slot_hold &) = delete;

  private:
    extract_slots &slots_;
    uint64_t ticket_;
    uint32_t d_;
};

} // namespace opencalibration_amd
