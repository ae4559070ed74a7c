// Contention on the scratch arenas' policy (deeppowers_amd/csrc/scratch_pool.h) without a device: 24 threads, each with its own stream key, over ONE pool and
// the logging backend of tools/scratch_pool_fake.h.  First every thread holds a lease at once (24 pinned arenas: creation beyond the cap of 16), then each
// takes 2000 leases of varying sizes (growth; eviction, since 24 streams share 16 places), every fourth thread releasing its own arena or all of them in
// between.  During a lease the worker writes its number into the block's header, yields and reads it back: a block freed under a lease is re-issued by the
// backend to the next caller, and shows.  Built through tests/cpp_build.py and run by tests/test_scratch_pool_cpu.py; exit code 0 = all checks passed.
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <thread>

#include "../../../tools/scratch_pool_fake.h"

using namespace scratch_fake;

static const int kThreads = 24, kLeases = 2000;
static std::atomic<long> failures{0};
#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { if (failures++ < 20) std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0, round = 0;
    void wait() {
        std::unique_lock<std::mutex> l(m);
        const int r = round;
        if (++waiting == kThreads) { waiting = 0; ++round; cv.notify_all(); }
        else cv.wait(l, [&] { return round != r; });
    }
};

// one lease: the block is live and this thread's alone while it lasts
static void lease_once(Pool& pool, State& st, uint64_t stream, size_t words, uint64_t id, Barrier* hold) {
    Pool::Lease l;
    const char* detail = "";
    const int rc = pool.acquire(stream, words, l, detail);
    CHECK(rc == DPFHE_SUCCESS);
    if (rc) return;
    st.mark_leased(l.p);
    l.p[0] = id;
    if (hold) hold->wait();
    std::this_thread::yield();
    CHECK(l.p[0] == id);
    CHECK(st.live(l.p));
    st.mark_ended(l.p);   // before the pool's end: from then on the block may leave
    pool.end(l);
}

int main() {
    State st;
    Barrier all_hold;
    std::atomic<size_t> most_arenas{0};
    {
        Pool pool{Backend{&st}};
        std::vector<std::thread> threads;
        for (int t = 0; t < kThreads; ++t)
            threads.emplace_back([&, t] {
                const uint64_t stream = 1000 + (uint64_t)t, id = (uint64_t)t + 1;
                lease_once(pool, st, stream, 1, id, &all_hold);   // every thread inside a lease at once
                uint64_t x = 88172645463325252ull * id;
                for (int i = 0; i < kLeases; ++i) {
                    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                    const size_t steps = 1 + (x >> 20) % 4;        // 1 ... 4 steps of 16 MiB: a larger request than the arena holds grows it
                    lease_once(pool, st, stream, steps * dpfhe::kScratchGranWords - (x & 1), id, nullptr);
                    const size_t now = pool.arenas();
                    for (size_t seen = most_arenas.load(); now > seen && !most_arenas.compare_exchange_weak(seen, now);) {}
                    if (t % 4 == 0 && i % 16 == 5) CHECK(pool.release(stream, false) == DPFHE_SUCCESS);   // its own arena: idle between its leases
                    if (t % 4 == 0 && i % 128 == 77) {
                        const int rc = pool.release(0, true);      // whatever is idle goes; an arena under another thread's lease stays
                        CHECK(rc == DPFHE_SUCCESS || rc == DPFHE_INVALID_STATE);
                    }
                }
            });
        for (auto& th : threads) th.join();
        CHECK(most_arenas.load() <= (size_t)kThreads);
        lease_once(pool, st, 1, 1, 99, nullptr);                   // one more creation: it evicts idle arenas down to the cap
        CHECK(pool.arenas() <= dpfhe::kMaxScratchArenas);
        CHECK(pool.release(0, true) == DPFHE_SUCCESS);
        CHECK(pool.bytes() == 0 && pool.arenas() == 0);
    }
    long allocs = 0, frees = 0, events = 0, destroyed = 0, most_live = 0, live = 0;
    for (const Entry& e : st.log) {
        allocs += e.op == kAlloc; frees += e.op == kFree; events += e.op == kNewEvent; destroyed += e.op == kDestroyEvent;
        live += (e.op == kNewEvent) - (e.op == kDestroyEvent);
        most_live = live > most_live ? live : most_live;
    }
    CHECK(st.errors == 0);
    CHECK(allocs == frees && events == destroyed && st.blocks.empty() && st.events.empty());
    CHECK(most_live >= kThreads);                                  // creation beyond the cap happened
    CHECK(destroyed > kThreads);                                   // ... and eviction or release
    CHECK(allocs > events);                                        // ... and growth (an allocation that is not an arena's first)
    std::printf("%d threads x %d leases: %ld arenas made, %ld allocations, most arenas at once %ld, backend errors %ld\n", kThreads, kLeases, events, allocs, most_live, st.errors);
    if (failures) { std::printf("%ld failures\n", failures.load()); return 1; }
    std::printf("arena threads OK\n");
    return 0;
}
