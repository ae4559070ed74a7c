"""The stream contract of one call: "runs on the caller's stream, only enqueues, does not allocate in steady state" (include/dpfhe.h, Conventions).
A plain helper like tests/footprint.py (no conftest, no plugin); tests/test_gpu_stream_gate.py shows on stand-in entries that it reports every planted
defect, tests/test_gpu_stream_contract.py runs the entry points of include/dpfhe.h and the C++ facade through it.

The gate (tests/cpp/stream_gate.hip, built into tests/cpp/libstream_gate.so on first use) is a kernel of one thread that holds a stream for a
requested time and touches no memory.  S is a NON-BLOCKING stream made with hipStreamCreateWithFlags: a blocking stream is implicitly ordered against
the null stream, so a stray null-stream launch would become ordered too and go unseen.

run_gated(gate, arena, expected, call) - the buffers laid out by a footprint.Arena, `expected` the oracle's words, call(t, stream) the entry on the
uploaded array t (an int64 tensor) with stream pointer `stream`:
  1. two uploads: TRUE (real inputs, PATTERNS[0] everywhere else) and WORK (the same with every input / inout region zeroed; zero is canonical for
     every kind of buffer the ABI takes);
  2. warm-up: the call on WORK with stream S, synchronise S - code objects loaded, the arena of S at its size, only zero-derived intermediates left;
  3. read scratch_bytes, synchronise the device;
  4. on S: the gate of length G, event E, WORK.copy_(TRUE) - the true inputs arrive only behind the gate, and the same copy wipes every output and
     scratch region back to the pattern;
  5. the call with stream S, timed on the host (t_enqueue);  6. closed = not E.query();
  7. the return code is success; the call came back while S was still held ('synchronised' if not: it waited for S or for the device); t_enqueue <= G / 4
     ('inconclusive' otherwise - a failure that reports both numbers, never a skip or a pass);
  8. synchronise S;  9. scratch_bytes unchanged ('allocated');
  10. Arena.verify and Arena.check_outputs against `expected` ('wrong' / 'unwritten'), guards and inputs as in footprint mode;
  11. if the case has an input region, the warm-up's outputs differed from `expected` in every output region: a case that cannot tell zero inputs from
      true ones cannot see a stray launch, and fails rather than passes quietly.
A launch on any stream other than S runs DURING the gate (the other stream is idle, nothing orders it): as the first kernel it reads zero inputs, in
the middle the warm-up's zero-derived intermediates, as the last kernel (or in an entry without inputs) its output is wiped by the copy behind the
gate.  In every position the final words differ from the oracle's.

A call that waited (E already complete when it returns) is reported as 'synchronised' even though its t_enqueue is then above G / 4 as well: a wait on
S lasts the whole gate, so the time alone cannot tell it from a slow host, E can.  'inconclusive' is a call that was slow while S was still held.

G (GATE_SECONDS) must be at least 10 ms and at least 20 x the slowest steady-state t_enqueue of the gated suite on the MI355X, so that a loaded host does
not turn into 'inconclusive'; Gate.slowest keeps that time and its case, MEASUREMENTS.md records what was measured.  The G / 4 assertion is what keeps a
too-short gate from hiding anything."""
import ctypes as C
import os
import subprocess
import time

import numpy as np

from footprint import PATTERNS, FootprintError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stream_gate.hip")
LIB = os.path.join(ROOT, "tests", "cpp", "libstream_gate.so")
TICK_HZ = 100_000_000            # wall_clock64() on gfx950
GATE_SECONDS = 0.040
MAX_PROBED = 8
KINDS = ("wrong", "unwritten", "synchronised", "allocated", "inconclusive")


class StreamContractError(AssertionError):
    """a violated stream contract: .kind is 'wrong' | 'unwritten' | 'synchronised' | 'allocated' | 'inconclusive'"""

    def __init__(self, kind, message):
        assert kind in KINDS, kind
        super().__init__(message)
        self.kind = kind


def build_library():
    """hipcc cross-compiles the gate for gfx950 (no GPU needed); rebuilt when the source is newer"""
    if not os.path.exists(LIB) or os.path.getmtime(SRC) > os.path.getmtime(LIB):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return LIB


def load():
    import torch  # noqa: F401  (loads the HIP runtime the library then resolves, as deeppowers_amd._cabi.load does)
    lib = C.CDLL(build_library())
    lib.stream_gate_enqueue.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    lib.stream_gate_stream_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.stream_gate_stream_destroy.argtypes = [C.c_void_p]
    return lib


class Gate:
    """a non-blocking stream S and the gate on it; .ptr the hipStream_t, .stream the torch.cuda.ExternalStream, .seconds G"""

    def __init__(self, lib, device, seconds=GATE_SECONDS):
        import torch
        self.lib, self.device, self.seconds = lib, torch.device(device), seconds
        p = C.c_void_p()
        rc = lib.stream_gate_stream_create(C.byref(p))
        assert rc == 0 and p.value, f"hipStreamCreateWithFlags(hipStreamNonBlocking): {rc}"
        self.ptr = int(p.value)
        self.stream = torch.cuda.ExternalStream(self.ptr, device=self.device)
        self.slowest = (0.0, "")             # the slowest steady-state t_enqueue of a case that passed, and its label
        self.cases = 0

    def hold(self, stream_ptr=None, seconds=None):
        """enqueue the gate; the iteration cap is 4 turns per microsecond asked for (a turn takes about one)"""
        seconds = self.seconds if seconds is None else seconds
        ticks = int(seconds * TICK_HZ)
        rc = self.lib.stream_gate_enqueue(C.c_void_p(self.ptr if stream_ptr is None else stream_ptr), ticks, max(4 * ticks // 100, 1))
        assert rc == 0, f"stream_gate_enqueue: {rc}"

    def measure(self):
        """the gate's real length in seconds, by two events on S"""
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.stream.synchronize()
        e0.record(self.stream)
        self.hold()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def close(self):
        import torch
        torch.cuda.synchronize(self.device)
        self.lib.stream_gate_stream_destroy(C.c_void_p(self.ptr))


def _zeroed_inputs(arena, buf):
    work = buf.copy()
    for r in arena.regions.values():
        if r.data is not None:
            for o, w in r.segments:
                work[r.offset + o: r.offset + o + w] = 0
    return work


def run_gated(gate, arena, expected, call, scratch_bytes=None, what=""):
    """the protocol of the module docstring; returns the array after the gated call"""
    import torch
    dev, S = gate.device, gate.stream
    G = gate.seconds
    true = arena.fill(PATTERNS[0])
    has_input = any(r.data is not None for r in arena.regions.values())
    TRUE = torch.from_numpy(true.view(np.int64)).to(dev)
    WORK = torch.from_numpy(_zeroed_inputs(arena, true).view(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    rc = call(WORK, gate.ptr)
    assert not rc, f"{what}: the warm-up call returned {rc}"
    S.synchronize()
    warm = WORK.cpu().numpy().view(np.uint64)
    held = scratch_bytes() if scratch_bytes else 0
    torch.cuda.synchronize(dev)
    E = torch.cuda.Event()
    gate.hold()
    E.record(S)
    with torch.cuda.stream(S):
        WORK.copy_(TRUE)
    t0 = time.perf_counter()
    rc = call(WORK, gate.ptr)
    t_enqueue = time.perf_counter() - t0
    closed = not E.query()
    try:
        assert not rc, f"{what}: the gated call returned {rc}"
        numbers = f"t_enqueue = {t_enqueue * 1e3:.3f} ms, G = {G * 1e3:.1f} ms"
        if not closed:
            raise StreamContractError("synchronised", f"{what}: the gate on S had ended when the call returned: the call waited for S or for the device "
                                                      f"(or the host took longer than the gate: {numbers})")
        if t_enqueue > G / 4:
            raise StreamContractError("inconclusive", f"{what}: the call took longer than G / 4 to return while S was held: {numbers}")
    finally:
        S.synchronize()
        torch.cuda.synchronize(dev)              # (a stray launch on another stream is over as well before the download)
    now = scratch_bytes() if scratch_bytes else 0
    if now != held:
        raise StreamContractError("allocated", f"{what}: the context's scratch arenas went from {held} to {now} bytes in steady state")
    after = WORK.cpu().numpy().view(np.uint64)
    try:
        arena.verify(after)
        arena.check_outputs(after, expected)
    except FootprintError as e:
        raise StreamContractError("unwritten" if e.kind == "unwritten" else "wrong",
                                  f"{what}: behind a gate on its own stream, with the inputs arriving after the gate: {e}") from e
    if has_input:
        for name, want in expected.items():
            if np.array_equal(arena.view(warm, name), np.ascontiguousarray(want, dtype=np.uint64).ravel()):
                raise StreamContractError("wrong", f"{what}: {name} after the warm-up on zero inputs already equals the expected words: this case cannot "
                                                   f"tell a launch that ran before the inputs arrived")
    gate.cases += 1
    if t_enqueue > gate.slowest[0]:
        gate.slowest = (t_enqueue, what)
    return after


# ---- stand-in entries: three chained torch ops on the arena's addresses (copy, add, copy), each on a stream of the test's choosing ---------------------
STANDIN_WORDS = 4096 + 6


def standin_arena(with_input=True):
    """in -> t1 (copy), t1 + in -> t2 (add), t2 -> out (copy): out = 2 * in (mod 2^64); without input: out = 7 everywhere"""
    from footprint import Arena
    ar = Arena()
    x = np.random.default_rng(11).integers(1, 1 << 62, STANDIN_WORDS, dtype=np.uint64)
    if with_input:
        ar.carve("in", STANDIN_WORDS, "input", STANDIN_WORDS, data=x)
        ar.carve("t1", STANDIN_WORDS, "scratch", STANDIN_WORDS)
        ar.carve("t2", STANDIN_WORDS, "scratch", STANDIN_WORDS)
    ar.carve("out", STANDIN_WORDS, "output", STANDIN_WORDS)
    return ar, {"out": x * np.uint64(2) if with_input else np.full(STANDIN_WORDS, 7, np.uint64)}


def standin_call(arena, device, streams=(None, None, None), before_return=None):
    """the stand-in entry as call(t, stream); streams[i]: the stream step i + 1 is issued on - None: the caller's, 'null': the null stream, or a
    torch stream; before_return(caller's torch stream) runs on the host after the three steps"""
    import torch

    def call(t, stream_ptr):
        caller = torch.cuda.ExternalStream(stream_ptr, device=device)
        pick = lambda s: caller if s is None else torch.cuda.default_stream(device) if s == "null" else s
        v = lambda name: t[arena.offset(name): arena.offset(name) + arena.regions[name].words]
        if "in" in arena.regions:
            steps = (lambda: v("t1").copy_(v("in")), lambda: torch.add(v("t1"), v("in"), out=v("t2")), lambda: v("out").copy_(v("t2")))
        else:
            steps = (lambda: v("out").fill_(7),)
        for step, s in zip(steps, streams):
            with torch.cuda.stream(pick(s)):
                step()
        if before_return:
            before_return(caller)
        return 0
    return call


_shared = {}


def shared_gate(device):
    """the gate every gated test of the process uses.  Nobody has measured how HIP places non-blocking streams on the hardware queues: were S to share
    a queue with the null stream, a stray null-stream launch would queue up behind the gate and go unseen.  So S is chosen by probing: of up to
    MAX_PROBED non-blocking streams, the first on which the planted defect 'step 1 on the null stream' is caught - and on which the correct stand-in
    passes.  None qualifying is an error (the gated tests then fail rather than pass vacuously).  The gate's measured length must lie between 0.5 x
    and 4 x the request."""
    if "gate" in _shared:
        return _shared["gate"]
    assert "error" not in _shared, _shared.get("error")
    lib = load()
    ar, want = standin_arena()
    probed, chosen = [], None
    for i in range(MAX_PROBED):
        g = Gate(lib, device)
        probed.append(g)
        try:
            run_gated(g, ar, want, standin_call(ar, g.device, ("null", None, None)), what=f"probe of stream {i}")
            continue                                                  # the defect went unseen on this stream
        except StreamContractError as e:
            if e.kind not in ("wrong", "unwritten"):
                continue
        try:
            run_gated(g, ar, want, standin_call(ar, g.device), what=f"probe of stream {i}, correct stand-in")
        except StreamContractError:
            continue
        chosen = i
        break
    if chosen is None:
        _shared["error"] = f"none of {len(probed)} non-blocking streams shows a stray null-stream launch behind the gate"
        raise AssertionError(_shared["error"])
    gate = probed[chosen]
    gate.probed_index = chosen
    gate.cases, gate.slowest = 0, (0.0, "")
    gate.measured = gate.measure()
    if not 0.5 * gate.seconds <= gate.measured <= 4 * gate.seconds:
        _shared["error"] = f"a gate of {gate.seconds * 1e3:.1f} ms measured {gate.measured * 1e3:.3f} ms"
        raise AssertionError(_shared["error"])
    _shared["gate"] = gate
    return gate
