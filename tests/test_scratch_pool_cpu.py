"""CPU: the policy of the per-stream scratch arenas (csrc/scratch_pool.h: leases, idle-only eviction, growth, release) over a backend that logs every
operation, keeps each block live or freed and counts misuse (tools/scratch_pool_fake.h), driven through ctypes (tools/emulate_scratch_pool.cpp); and the
same pool under 24 contending threads in a stand-alone program (tests/cpp/arenas/arena_threads.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

import cpp_build

ROOT = cpp_build.ROOT
ALLOC, FREE, NEW_EVENT, DESTROY_EVENT, RECORD, WAIT = 1, 2, 3, 4, 5, 6     # tools/scratch_pool_fake.h Op
SUCCESS, OUT_OF_MEMORY, INVALID_STATE = 0, 1001, 2002                    # include/dpfhe.h
CAP = 16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_scratch_pool.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, os.path.join(ROOT, "tools", "emulate_scratch_pool.cpp")])
    lib = C.CDLL(so)
    lib.emu_pool_new.restype = C.c_void_p
    lib.emu_pool_delete.argtypes = [C.c_void_p]
    lib.emu_pool_gran_words.restype = C.c_uint64
    lib.emu_pool_acquire.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    lib.emu_pool_end.argtypes = [C.c_void_p, C.c_int]
    lib.emu_pool_release.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    for name in ("emu_pool_bytes", "emu_pool_arenas"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p], C.c_uint64
    lib.emu_pool_detail.argtypes, lib.emu_pool_detail.restype = [C.c_void_p], C.c_char_p
    lib.emu_pool_errors.argtypes, lib.emu_pool_errors.restype = [C.c_void_p], C.c_long
    lib.emu_pool_block_live.argtypes = [C.c_void_p, C.c_uint64]
    lib.emu_pool_fail_allocs.argtypes = [C.c_void_p, C.c_long]
    lib.emu_pool_log.argtypes, lib.emu_pool_log.restype = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64], C.c_uint64
    lib.emu_pool_log_clear.argtypes = [C.c_void_p]
    assert lib.emu_pool_cap() == CAP and lib.emu_pool_gran_words() * 8 == 16 << 20
    return lib


class Pool:
    """one emulated pool; streams are numbers from 1"""

    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p(lib.emu_pool_new())
        self.gran = lib.emu_pool_gran_words()

    def close(self):
        self.lib.emu_pool_delete(self.h)

    def acquire(self, stream, words=1):
        """(result code, lease number, block)"""
        lease, block = C.c_int(-1), C.c_uint64(0)
        rc = self.lib.emu_pool_acquire(self.h, stream, words, C.byref(lease), C.byref(block))
        return rc, lease.value, block.value

    def lease(self, stream, words=1):
        rc, lease, block = self.acquire(stream, words)
        assert rc == SUCCESS, (rc, self.lib.emu_pool_detail(self.h))
        return lease, block

    def use(self, stream, words=1):
        """a whole call: lease, end; the block it ran on"""
        lease, block = self.lease(stream, words)
        self.end(lease)
        return block

    def end(self, lease):
        self.lib.emu_pool_end(self.h, lease)

    def release(self, stream=0, all_streams=False):
        return self.lib.emu_pool_release(self.h, stream, int(all_streams))

    def live(self, block):
        return bool(self.lib.emu_pool_block_live(self.h, block))

    arenas = property(lambda self: self.lib.emu_pool_arenas(self.h))
    bytes = property(lambda self: self.lib.emu_pool_bytes(self.h))
    errors = property(lambda self: self.lib.emu_pool_errors(self.h))

    def log(self, clear=True):
        n = self.lib.emu_pool_log(self.h, None, 0)
        buf = (C.c_uint64 * (3 * n))()
        self.lib.emu_pool_log(self.h, buf, n)
        if clear:
            self.lib.emu_pool_log_clear(self.h)
        return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]


@pytest.fixture
def pool(lib):
    p = Pool(lib)
    yield p
    assert p.errors == 0
    p.close()


def departures(log):
    """the blocks that left, in order, each checked to have gone by wait(its event), free(block), destroy_event(that event) with nothing in between"""
    gone = []
    for i, (op, a, _) in enumerate(log):
        if op == FREE:
            assert log[i - 1][0] == WAIT and log[i + 1][:2] == (DESTROY_EVENT, log[i - 1][1]), log[i - 1:i + 2]
            gone.append(a)
    assert sum(op == WAIT for op, _, _ in log) == len(gone) == sum(op == DESTROY_EVENT for op, _, _ in log)
    return gone


def test_sequential_rotation_keeps_the_cap_and_evicts_the_least_recently_used(pool):
    blocks = []
    for i in range(20):
        stream = i + 1
        lease, block = pool.lease(stream)
        log = pool.log()
        assert [e for e in log if e[0] in (NEW_EVENT, ALLOC)] == [(NEW_EVENT, log[-2][1], 0), (ALLOC, block, pool.gran)]
        assert all(op != RECORD for op, _, _ in log)                              # nothing in a lease's beginning takes a stream
        assert departures(log) == ([blocks[i - CAP]] if i >= CAP else [])       # streams were used once each, in order: the oldest is the LRU
        if i >= CAP:
            assert log.index((FREE, blocks[i - CAP], 0)) < log.index((ALLOC, block, pool.gran)) and not pool.live(blocks[i - CAP])
        pool.end(lease)
        assert pool.log() == [(RECORD, log[-2][1], stream)]                       # the only operation that takes a stream, and it is the caller's own
        blocks.append(block)
        assert pool.arenas == min(i + 1, CAP) and pool.bytes == pool.gran * 8 * min(i + 1, CAP)
    # the table holds streams 5 ... 20; a second use moves stream 5 to the back of the queue: the next new stream evicts 6
    assert pool.use(5) == blocks[4]
    pool.log()
    pool.use(21)
    assert departures(pool.log()) == [blocks[5]] and pool.live(blocks[4])


def test_a_leased_arena_is_never_the_victim(pool):
    blocks = {s: pool.use(s) for s in range(1, CAP + 1)}
    lease, block = pool.lease(1)                                    # the least recently used arena, now in use
    assert block == blocks[1]
    pool.log()
    pool.use(CAP + 1)
    assert departures(pool.log()) == [blocks[2]]                    # the least recently used IDLE one
    assert pool.live(blocks[1]) and pool.arenas == CAP
    pool.end(lease)
    pool.log()
    pool.use(CAP + 2)                                               # 1 was used last: 3 goes
    assert departures(pool.log()) == [blocks[3]] and pool.live(blocks[1])


@pytest.mark.parametrize("seventeenth_ends_first", (True, False))
def test_all_leased_goes_beyond_the_cap_and_comes_back(pool, seventeenth_ends_first):
    held = [pool.lease(s) for s in range(1, CAP + 1)]
    pool.log()
    lease17, block17 = pool.lease(CAP + 1)
    assert departures(pool.log()) == [] and pool.arenas == CAP + 1
    assert all(pool.live(b) for _, b in held)
    if seventeenth_ends_first:
        pool.end(lease17)
    for lease, _ in held:                                           # ended in the order 1 ... 16
        pool.end(lease)
    if not seventeenth_ends_first:
        pool.end(lease17)
    pool.log()
    pool.use(CAP + 2)                                               # the two whose leases ended first are the two least recently used
    assert departures(pool.log()) == ([block17, held[0][1]] if seventeenth_ends_first else [held[0][1], held[1][1]]) and pool.arenas == CAP


def test_growth_waits_frees_then_allocates_in_16_mib_steps(pool):
    small = pool.use(7, 1)
    creation = pool.log()
    event = [a for op, a, _ in creation if op == NEW_EVENT][0]
    assert pool.use(7, pool.gran) == small and pool.log() == [(RECORD, event, 7)]          # fits: the same block, nothing but the record
    lease, big = pool.lease(7, pool.gran + 1)
    assert pool.log() == [(WAIT, event, 0), (FREE, small, 0), (ALLOC, big, 2 * pool.gran)]
    assert pool.bytes == 2 * pool.gran * 8 and pool.arenas == 1
    # a second lease of the same arena that fits shares it; one that does not is refused while the first lasts, and nothing moves
    lease2, same = pool.lease(7, 5)
    assert same == big
    rc, _, _ = pool.acquire(7, 2 * pool.gran + 1)
    assert rc == INVALID_STATE and pool.log() == [] and pool.bytes == 2 * pool.gran * 8 and pool.live(big)
    pool.end(lease2)
    rc, _, _ = pool.acquire(7, 2 * pool.gran + 1)
    assert rc == INVALID_STATE and pool.live(big)
    pool.end(lease)
    pool.log()
    pool.use(7, 2 * pool.gran + 1)
    assert [e[0] for e in pool.log()] == [WAIT, FREE, ALLOC, RECORD] and pool.bytes == 3 * pool.gran * 8


def test_release_of_one_stream_and_of_all(pool):
    blocks = {s: pool.use(s) for s in (1, 2, 3, 4)}
    pool.log()
    assert pool.release(9) == SUCCESS and pool.log() == []          # a stream without an arena
    assert pool.release(2) == SUCCESS
    assert departures(pool.log()) == [blocks[2]] and pool.arenas == 3
    lease, block = pool.lease(3)
    pool.log()
    assert pool.release(3) == INVALID_STATE and pool.log() == [] and pool.live(blocks[3])
    assert pool.release(all_streams=True) == INVALID_STATE          # the others go, the pinned one stays
    assert sorted(departures(pool.log())) == sorted([blocks[1], blocks[4]]) and pool.live(blocks[3]) and pool.arenas == 1
    assert pool.bytes == pool.gran * 8
    pool.end(lease)
    pool.log()
    assert pool.release(all_streams=True) == SUCCESS
    assert departures(pool.log()) == [blocks[3]] and pool.arenas == 0 and pool.bytes == 0
    assert pool.release(all_streams=True) == SUCCESS


def test_allocation_failure_leaves_the_table_and_no_pin(pool):
    blocks = {s: pool.use(s) for s in range(1, CAP + 1)}
    pool.log()
    pool.lib.emu_pool_fail_allocs(pool.h, 1)
    rc, _, _ = pool.acquire(CAP + 1)                                # creation: the victim is gone already, the new arena never appears
    assert rc == OUT_OF_MEMORY and b"out of memory" in pool.lib.emu_pool_detail(pool.h)
    log = pool.log()
    assert [e[0] for e in log] == [WAIT, FREE, DESTROY_EVENT, NEW_EVENT, DESTROY_EVENT] and log[1][1] == blocks[1]
    assert pool.arenas == CAP - 1 and pool.bytes == pool.gran * 8 * (CAP - 1)
    pool.lib.emu_pool_fail_allocs(pool.h, 1)
    rc, _, _ = pool.acquire(5, pool.gran + 1)                       # growth: the old block is gone, the arena stays, empty and idle
    assert rc == OUT_OF_MEMORY and [e[0] for e in pool.log()] == [WAIT, FREE]
    assert pool.arenas == CAP - 1 and pool.bytes == pool.gran * 8 * (CAP - 2)
    assert pool.use(5, pool.gran + 1) and pool.bytes == pool.gran * 8 * CAP     # not left pinned: it grows now ...
    assert pool.release(all_streams=True) == SUCCESS and pool.arenas == 0       # ... and everything can be released


def test_the_mutex_is_not_held_across_wait_and_free(lib):
    assert lib.emu_pool_wait_leaves_the_mutex(5000) == 1


def test_threads_contend_for_one_pool():
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "arenas"), exist_ok=True)   # (cpp_build makes tests/cpp/bin but no directory below it)
    exe = cpp_build.build_program("arenas/arena_threads", extra_flags=("-pthread",))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "arena threads OK" in out.stdout, out.stdout + out.stderr
