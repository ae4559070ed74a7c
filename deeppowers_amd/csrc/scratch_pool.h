// scratch_pool.h - the policy of the per-stream scratch arenas of the composed operations (cabi.h StreamScratch), host only and free of HIP: the table of
// arenas, its mutex, the LRU clock and the cap.  The device calls are the Backend's (cabi_ctx.hip HipScratchBackend; a logging fake in
// tools/emulate_scratch_pool.cpp, which tests/test_scratch_pool_cpu.py and tests/cpp/arenas/arena_threads.cpp drive), and there are exactly these:
//   int alloc(size_t words, uint64_t*& p, const char*& detail)    0, or an error code of dpfhe.h with its text
//   void free(uint64_t* p)
//   int new_event(Event& e, const char*& detail);  void destroy_event(Event e)
//   void record(Event e, Stream s)                                 the event completes when everything enqueued on s so far has run
//   void wait(Event e)                                             blocks the host until the event's last record has completed
// The pool never synchronises a stream: a stream handle is the key of its arena and, while its owner is inside a call, the argument of record - so the
// owner may destroy the stream as soon as its calls have returned.
//
// One ARENA per stream that ran a composed operation: a plain device allocation in 16 MiB steps, kept until release, eviction or the pool's end, grown
// only when a larger request than ever before arrives.  Work on one stream is ordered, so consecutive calls share their stream's arena without a fence.
//   Lease.     acquire() returns the block PINNED (pin count raised under the mutex).  end() first records the arena's one event on the stream, then
//              takes the mutex, unpins and stamps last_use: no thread sees an idle arena whose last work the event does not cover.
//   Eviction.  A new arena at the cap (kMaxScratchArenas) takes the place of the least recently used IDLE one, which leaves the table under the mutex and
//              is waited for (its event), freed and stripped of its event with the mutex released.  With every arena pinned the table grows beyond the
//              cap; every later creation evicts idle arenas while the table is at or above it.
//   Growth.    wait(event), free, alloc - on an arena no other lease pins (DPFHE_INVALID_STATE otherwise, nothing freed).
//   Release.   Idle arenas of one stream or of all leave as evicted ones do; a pinned arena stays and the call returns DPFHE_INVALID_STATE.
// An arena being created or grown stays in the table, pinned and empty, while its device calls run outside the mutex.
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/dpfhe.h"

namespace dpfhe {

static const size_t kMaxScratchArenas = 16;
static const size_t kScratchGranWords = (size_t)1 << 21;   // 16 MiB steps

template <class Backend>
class ScratchPool {
public:
    using Stream = typename Backend::Stream;
    using Event = typename Backend::Event;
    struct Lease { Stream stream{}; uint64_t* p = nullptr; Event event{}; };

    explicit ScratchPool(Backend b = Backend{}) : be_(b) {}
    ~ScratchPool() { dispose(arenas_); }
    ScratchPool(const ScratchPool&) = delete;
    ScratchPool& operator=(const ScratchPool&) = delete;

    int acquire(Stream s, size_t words, Lease& lease, const char*& detail) {
        std::vector<Arena> victims;
        uint64_t* old = nullptr;
        Event ev{};
        bool fresh = false;
        {
            std::lock_guard<std::mutex> lock(mutex_);
            Arena* a = find(s);
            if (a && a->words >= words) { ++a->pins; lease = Lease{s, a->p, a->event}; return DPFHE_SUCCESS; }
            if (a && a->pins) { detail = "the stream's arena is too small and in use by another call"; return DPFHE_INVALID_STATE; }
            if (a) { old = a->p; ev = a->event; a->p = nullptr; a->words = 0; a->pins = 1; }
            else {
                take_idle(victims, [&](const Arena&) { return arenas_.size() >= kMaxScratchArenas; });
                arenas_.push_back(Arena{s, nullptr, 0, ++clock_, 1, Event{}});
                fresh = true;
            }
        }
        dispose(victims);
        int rc = DPFHE_SUCCESS;
        if (fresh) rc = be_.new_event(ev, detail);
        else { be_.wait(ev); if (old) be_.free(old); }
        const bool own_event = fresh && rc == DPFHE_SUCCESS;
        const size_t want = (words + kScratchGranWords - 1) / kScratchGranWords * kScratchGranWords;
        uint64_t* p = nullptr;
        if (rc == DPFHE_SUCCESS) rc = be_.alloc(want, p, detail);
        {
            std::lock_guard<std::mutex> lock(mutex_);
            Arena* a = find(s);   // still there: pinned since the first section
            if (rc == DPFHE_SUCCESS) { a->p = p; a->words = want; a->event = ev; lease = Lease{s, p, ev}; }
            else if (fresh) arenas_.erase(arenas_.begin() + (a - arenas_.data()));
            else a->pins = 0;
        }
        if (rc != DPFHE_SUCCESS && own_event) be_.destroy_event(ev);
        return rc;
    }

    void end(const Lease& lease) {
        be_.record(lease.event, lease.stream);
        std::lock_guard<std::mutex> lock(mutex_);
        Arena* a = find(lease.stream);
        --a->pins;
        a->last_use = ++clock_;
    }

    // the arena of `s`, or every arena (all); DPFHE_INVALID_STATE when one of them is pinned (it stays)
    int release(Stream s, bool all) {
        std::vector<Arena> victims;
        bool busy = false;
        {
            std::lock_guard<std::mutex> lock(mutex_);
            for (const Arena& a : arenas_) busy = busy || ((all || a.stream == s) && a.pins);
            take_idle(victims, [&](const Arena& a) { return all || a.stream == s; });
        }
        dispose(victims);
        return busy ? DPFHE_INVALID_STATE : DPFHE_SUCCESS;
    }

    size_t bytes() const {
        std::lock_guard<std::mutex> lock(mutex_);
        size_t w = 0;
        for (const Arena& a : arenas_) w += a.words;
        return w * sizeof(uint64_t);
    }
    size_t arenas() const {
        std::lock_guard<std::mutex> lock(mutex_);
        return arenas_.size();
    }
    Backend& backend() { return be_; }

private:
    struct Arena { Stream stream; uint64_t* p; size_t words; uint64_t last_use; unsigned pins; Event event; };

    Arena* find(Stream s) {
        for (Arena& a : arenas_) if (a.stream == s) return &a;
        return nullptr;
    }
    // moves idle arenas that `take` accepts into `out`, least recently used first (one at a time: `take` may look at the table's size)
    template <class Take>
    void take_idle(std::vector<Arena>& out, Take take) {
        for (;;) {
            size_t lru = arenas_.size();
            for (size_t i = 0; i < arenas_.size(); ++i)
                if (!arenas_[i].pins && take(arenas_[i]) && (lru == arenas_.size() || arenas_[i].last_use < arenas_[lru].last_use)) lru = i;
            if (lru == arenas_.size()) return;
            out.push_back(arenas_[lru]);
            arenas_.erase(arenas_.begin() + (long)lru);
        }
    }
    // what leaves the table, with the mutex released: wait for its last recorded work, free the block, destroy the event
    void dispose(std::vector<Arena>& gone) {
        for (Arena& a : gone) {
            if (a.event == Event{}) continue;   // (created but never completed: nothing on the device yet)
            be_.wait(a.event);
            if (a.p) be_.free(a.p);
            be_.destroy_event(a.event);
        }
        gone.clear();
    }

    Backend be_;
    mutable std::mutex mutex_;
    std::vector<Arena> arenas_;
    uint64_t clock_ = 0;
};

}  // namespace dpfhe
