// A backend of csrc/scratch_pool.h without a device: it logs every operation in order, keeps each block live or freed, and counts as an ERROR any free of a
// block that is under a lease, any wait, record or destroy on an event that does not exist (any more), and any free of a block that is not live.  Blocks are
// 64 bytes of host memory whatever their size in words, and a freed block's memory is the next one handed out: a block freed under a lease is re-issued to
// the next caller, whose words the leaseholder then reads.  The log names a block by a serial number that is never issued twice.
// Shared by tools/emulate_scratch_pool.cpp (ctypes: tests/test_scratch_pool_cpu.py) and tests/cpp/arenas/arena_threads.cpp.  Host-only C++17.
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "../deeppowers_amd/csrc/scratch_pool.h"

namespace scratch_fake {

enum Op : int { kAlloc = 1, kFree, kNewEvent, kDestroyEvent, kRecord, kWait };
struct Entry { int op; uint64_t a, b; };   // alloc: (block's serial number, words)  free: (serial number, 0)  new / destroy / wait: (event, 0)  record: (event, stream)

struct State {
    std::mutex m;
    std::vector<Entry> log;
    bool keep_log = true;
    struct Block { uint64_t serial; int leases; };
    std::map<uint64_t*, Block> blocks;     // the live blocks, with the leases on them right now (mark_leased / mark_ended: the caller's, around a pool lease)
    uint64_t next_serial = 0;
    std::vector<uint64_t*> spare, all;     // freed memory, handed out again last-freed first; everything ever made
    std::set<int> events;
    int next_event = 0;
    long errors = 0, fail_allocs = 0;      // fail_allocs: that many coming allocations fail
    void (*on_wait)(void*, int) = nullptr; // called by wait(), outside this mutex (a test blocks in it)
    void* on_wait_arg = nullptr;
    ~State() { for (uint64_t* p : all) delete[] p; }
    void note(int op, uint64_t a, uint64_t b) { if (keep_log) log.push_back(Entry{op, a, b}); }
    void mark_leased(uint64_t* p) { std::lock_guard<std::mutex> l(m); auto it = blocks.find(p); if (it == blocks.end()) ++errors; else ++it->second.leases; }
    void mark_ended(uint64_t* p) { std::lock_guard<std::mutex> l(m); auto it = blocks.find(p); if (it == blocks.end() || it->second.leases == 0) ++errors; else --it->second.leases; }
    bool live(uint64_t* p) { std::lock_guard<std::mutex> l(m); return blocks.count(p) != 0; }
    uint64_t serial(uint64_t* p) { std::lock_guard<std::mutex> l(m); auto it = blocks.find(p); return it == blocks.end() ? 0 : it->second.serial; }
    bool live_serial(uint64_t serial) { std::lock_guard<std::mutex> l(m); for (auto& b : blocks) if (b.second.serial == serial) return true; return false; }
};

struct Backend {
    using Stream = uint64_t;
    using Event = int;   // 0: none
    State* st;
    int alloc(size_t words, uint64_t*& p, const char*& detail) {
        std::lock_guard<std::mutex> l(st->m);
        if (st->fail_allocs > 0) { --st->fail_allocs; detail = "out of memory (the fake backend was told to fail)"; return DPFHE_OUT_OF_MEMORY; }
        if (st->spare.empty()) { p = new uint64_t[8](); st->all.push_back(p); }
        else { p = st->spare.back(); st->spare.pop_back(); }
        st->blocks[p] = State::Block{++st->next_serial, 0};
        st->note(kAlloc, st->next_serial, words);
        return DPFHE_SUCCESS;
    }
    void free(uint64_t* p) {
        std::lock_guard<std::mutex> l(st->m);
        auto it = st->blocks.find(p);
        st->note(kFree, it == st->blocks.end() ? 0 : it->second.serial, 0);
        if (it == st->blocks.end() || it->second.leases != 0) { ++st->errors; return; }
        st->blocks.erase(it);
        st->spare.push_back(p);
    }
    int new_event(Event& e, const char*&) {
        std::lock_guard<std::mutex> l(st->m);
        e = ++st->next_event;
        st->events.insert(e);
        st->note(kNewEvent, (uint64_t)e, 0);
        return DPFHE_SUCCESS;
    }
    void destroy_event(Event e) {
        std::lock_guard<std::mutex> l(st->m);
        st->note(kDestroyEvent, (uint64_t)e, 0);
        if (!st->events.erase(e)) ++st->errors;
    }
    void record(Event e, Stream s) {
        std::lock_guard<std::mutex> l(st->m);
        st->note(kRecord, (uint64_t)e, s);
        if (!st->events.count(e)) ++st->errors;
    }
    void wait(Event e) {
        {
            std::lock_guard<std::mutex> l(st->m);
            st->note(kWait, (uint64_t)e, 0);
            if (!st->events.count(e)) ++st->errors;
        }
        if (st->on_wait) st->on_wait(st->on_wait_arg, e);
    }
};

using Pool = dpfhe::ScratchPool<Backend>;

}  // namespace scratch_fake
