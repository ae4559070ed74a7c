// CPU emulation of the scratch arenas' policy (csrc/scratch_pool.h) over the logging backend of tools/scratch_pool_fake.h, for ctypes
// (tests/test_scratch_pool_cpu.py):  g++ -O2 -std=c++17 -shared -fPIC -pthread -o libemu_scratch_pool.so tools/emulate_scratch_pool.cpp
// A handle is one pool with its backend state and the leases the caller holds on it (by number).
#include <chrono>
#include <condition_variable>
#include <thread>

#include "scratch_pool_fake.h"

using namespace scratch_fake;

namespace {
struct Emu {
    State st;   // (outlives the pool, whose end frees what is left through it)
    Pool pool{Backend{&st}};
    std::map<int, Pool::Lease> leases;
    int next_lease = 0;
    const char* detail = "";
};
}  // namespace

extern "C" {
void* emu_pool_new() { return new Emu; }
void emu_pool_delete(void* h) { delete static_cast<Emu*>(h); }
int emu_pool_cap() { return (int)dpfhe::kMaxScratchArenas; }
uint64_t emu_pool_gran_words() { return dpfhe::kScratchGranWords; }

// a lease of `words` for `stream`: the result code; on success the lease's number and its block's serial number
int emu_pool_acquire(void* h, uint64_t stream, uint64_t words, int* lease, uint64_t* block) {
    Emu* e = static_cast<Emu*>(h);
    Pool::Lease l;
    e->detail = "";
    const int rc = e->pool.acquire(stream, words, l, e->detail);
    if (rc) return rc;
    e->st.mark_leased(l.p);
    e->leases[*lease = e->next_lease++] = l;
    *block = e->st.serial(l.p);
    return 0;
}
void emu_pool_end(void* h, int lease) {
    Emu* e = static_cast<Emu*>(h);
    const Pool::Lease l = e->leases.at(lease);
    e->leases.erase(lease);
    e->st.mark_ended(l.p);   // before the pool's end: from then on the block may leave
    e->pool.end(l);
}
int emu_pool_release(void* h, uint64_t stream, int all) { return static_cast<Emu*>(h)->pool.release(stream, all != 0); }
uint64_t emu_pool_bytes(void* h) { return static_cast<Emu*>(h)->pool.bytes(); }
uint64_t emu_pool_arenas(void* h) { return static_cast<Emu*>(h)->pool.arenas(); }
const char* emu_pool_detail(void* h) { return static_cast<Emu*>(h)->detail; }
long emu_pool_errors(void* h) { return static_cast<Emu*>(h)->st.errors; }
int emu_pool_block_live(void* h, uint64_t block) { return static_cast<Emu*>(h)->st.live_serial(block) ? 1 : 0; }
void emu_pool_fail_allocs(void* h, long n) { static_cast<Emu*>(h)->st.fail_allocs = n; }
// the log so far as (op, a, b) triples (scratch_pool_fake.h Op); returns the number of entries, copies at most `cap` of them
uint64_t emu_pool_log(void* h, uint64_t* out, uint64_t cap) {
    State& st = static_cast<Emu*>(h)->st;
    std::lock_guard<std::mutex> l(st.m);
    for (size_t i = 0; i < st.log.size() && i < cap; ++i) { out[3 * i] = (uint64_t)st.log[i].op; out[3 * i + 1] = st.log[i].a; out[3 * i + 2] = st.log[i].b; }
    return st.log.size();
}
void emu_pool_log_clear(void* h) {
    State& st = static_cast<Emu*>(h)->st;
    std::lock_guard<std::mutex> l(st.m);
    st.log.clear();
}

// The mutex is not held across wait / free: 16 idle arenas, then thread A brings a 17th stream and its eviction's wait() blocks until thread B's acquire on
// another stream (an arena that stays) has RETURNED.  1: it did; 0: wait() gave up after `timeout_ms` (B was stuck behind the pool's mutex).
int emu_pool_wait_leaves_the_mutex(int timeout_ms) {
    struct Sync { std::mutex m; std::condition_variable cv; bool in_wait = false, b_done = false, saw_b = false; int timeout_ms; } sy;
    sy.timeout_ms = timeout_ms;
    Emu e;
    for (uint64_t s = 1; s <= dpfhe::kMaxScratchArenas; ++s) {
        Pool::Lease l;
        if (e.pool.acquire(s, 1, l, e.detail)) return -1;
        e.pool.end(l);
    }
    e.st.on_wait_arg = &sy;
    e.st.on_wait = [](void* arg, int) {
        Sync& y = *static_cast<Sync*>(arg);
        std::unique_lock<std::mutex> l(y.m);
        y.in_wait = true;
        y.cv.notify_all();
        y.saw_b = y.cv.wait_for(l, std::chrono::milliseconds(y.timeout_ms), [&] { return y.b_done; });
    };
    std::thread a([&] { Pool::Lease l; const char* d = ""; if (e.pool.acquire(100, 1, l, d) == 0) e.pool.end(l); });
    std::thread b([&] {
        { std::unique_lock<std::mutex> l(sy.m); sy.cv.wait_for(l, std::chrono::milliseconds(sy.timeout_ms), [&] { return sy.in_wait; }); }
        Pool::Lease l;
        const char* d = "";
        const int rc = e.pool.acquire(dpfhe::kMaxScratchArenas, 1, l, d);   // the most recently used stream: not the victim
        { std::lock_guard<std::mutex> g(sy.m); sy.b_done = true; }
        sy.cv.notify_all();
        if (rc == 0) e.pool.end(l);
    });
    a.join();
    b.join();
    e.st.on_wait = nullptr;
    return sy.saw_b && e.st.errors == 0 ? 1 : 0;
}
}
