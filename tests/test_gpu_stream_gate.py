"""The stream gate (tests/stream_gate.py) against planted defects: a CPU test that the gate kernel cross-compiles and exports its symbol, and, -m gpu,
stand-in "entries" of three chained torch ops on the arena's addresses (copy, add, copy) with one defect each.  None of the defects is a GPU fault, only a
misordered or waiting op; every one must be reported with its kind, and the correct stand-in must pass.  tests/test_gpu_stream_contract.py means
nothing unless these pass.

Which kind a misplaced step gives follows from the protocol (the stray step runs during the gate; the copy behind the gate then wipes scratch and output):
  step 1 (in -> t1) elsewhere: t1 is wiped to the fill pattern, step 2 adds the input to it                          -> 'wrong'
  step 2 (t1 + in -> t2) elsewhere: t2 is wiped, step 3 copies the pattern to out                                     -> 'unwritten'
  step 3 (t2 -> out) elsewhere, or a writer without inputs elsewhere: out is wiped and never written again            -> 'unwritten'"""
import ctypes as C
import subprocess
import time

import pytest

import stream_gate as sg


def test_gate_library_compiles_for_gfx950_and_exports_its_symbols():
    """CPU: hipcc cross-compiles tests/cpp/stream_gate.hip; the library exports stream_gate_enqueue and carries a gfx950 code object"""
    so = sg.build_library()
    names = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for symbol in ("stream_gate_enqueue", "stream_gate_stream_create", "stream_gate_stream_destroy"):
        assert f" T {symbol}" in names, names
    assert b"gfx950" in open(so, "rb").read()
    src = open(sg.SRC).read()
    assert "*" not in src.split("__global__")[1].split(")")[0], "the gate kernel takes no pointer"


def test_error_kinds():
    """CPU: the error carries its kind and refuses an unknown one"""
    assert sg.StreamContractError("allocated", "x").kind == "allocated" and issubclass(sg.StreamContractError, AssertionError)
    with pytest.raises(AssertionError):
        sg.StreamContractError("slow", "x")


@pytest.fixture(scope="module")
def gate():
    return sg.shared_gate("cuda:0")


@pytest.fixture(scope="module")
def second_stream(gate):
    import torch
    p = C.c_void_p()
    assert gate.lib.stream_gate_stream_create(C.byref(p)) == 0
    yield torch.cuda.ExternalStream(int(p.value), device=gate.device)
    torch.cuda.synchronize(gate.device)
    gate.lib.stream_gate_stream_destroy(p)


def _run(gate, streams=(None, None, None), before_return=None, with_input=True):
    ar, want = sg.standin_arena(with_input)
    return sg.run_gated(gate, ar, want, sg.standin_call(ar, gate.device, streams, before_return), what="stand-in")


@pytest.mark.gpu
def test_gate_length_and_probe(gate):
    """a stream qualified, and the gate's measured length is within 0.5 x ... 4 x of the request (shared_gate raises otherwise); a request beyond the
    caps is refused without a launch"""
    print(f"\nstream gate: G = {gate.seconds * 1e3:.1f} ms requested, {gate.measured * 1e3:.3f} ms measured; probed stream {gate.probed_index} qualified")
    assert 0 <= gate.probed_index < sg.MAX_PROBED
    assert 0.5 * gate.seconds <= gate.measured <= 4 * gate.seconds
    assert gate.seconds >= 0.010
    assert gate.lib.stream_gate_enqueue(C.c_void_p(gate.ptr), 10 ** 9, 1000) == -1
    assert gate.lib.stream_gate_enqueue(C.c_void_p(gate.ptr), 1000, 10 ** 9) == -1


@pytest.mark.gpu
def test_correct_standins_pass(gate):
    _run(gate)
    _run(gate, (None,), with_input=False)


@pytest.mark.gpu
@pytest.mark.parametrize("step,kind", [(0, "wrong"), (1, "unwritten"), (2, "unwritten")])
@pytest.mark.parametrize("where", ["null", "second"])
def test_a_step_on_another_stream_is_caught(gate, second_stream, where, step, kind):
    streams = [None, None, None]
    streams[step] = "null" if where == "null" else second_stream
    with pytest.raises(sg.StreamContractError) as e:
        _run(gate, tuple(streams))
    assert e.value.kind == kind, e.value


@pytest.mark.gpu
def test_an_input_free_writer_on_the_null_stream_is_caught(gate):
    with pytest.raises(sg.StreamContractError) as e:
        _run(gate, ("null",), with_input=False)
    assert e.value.kind == "unwritten", e.value


@pytest.mark.gpu
def test_waiting_for_the_stream_or_the_device_is_caught(gate):
    import torch
    for wait in (lambda s: s.synchronize(), lambda s: torch.cuda.synchronize(gate.device)):
        with pytest.raises(sg.StreamContractError) as e:
            _run(gate, before_return=wait)
        assert e.value.kind == "synchronised", e.value


@pytest.mark.gpu
def test_a_slow_host_is_inconclusive_not_a_pass(gate):
    """a host sleep of 0.3 G: longer than G / 4, over before the gate ends"""
    with pytest.raises(sg.StreamContractError) as e:
        _run(gate, before_return=lambda s: time.sleep(0.3 * gate.seconds))
    assert e.value.kind == "inconclusive", e.value


@pytest.mark.gpu
def test_arena_growth_in_the_gated_call_is_caught(gate):
    """a composed dpfhe_ct_mul at N = 16384 whose gated call has a larger batch than its warm-up: the arena of S grows, which synchronises S.  The
    arena grows in steps of 16 MiB and the multiply takes 4 L N words = 2 MiB per item here: batch 1 leaves room for 8 items, batch 9 needs more"""
    import test_gpu_footprint as fp
    r = fp.make_rig("fold", 14)
    try:
        lib, h, poly = r.ctx._lib, r.ctx.handle, r.L * r.n
        label, a, b, flags, want = next(c for c in fp.ct_mul_cases(r, (9,), ()) if c[3] == 0)
        c = fp.Case(r)
        c.inp("a2", a, 2 * poly)
        c.inp("b2", b, 2 * poly)
        c.out("out3", 9 * 3 * poly, 3 * poly, want)
        batches = iter((1, 9))
        with pytest.raises(sg.StreamContractError) as e:
            c.run_gated(label, lambda at: lib.dpfhe_ct_mul(h, at("out3"), at("a2"), at("b2"), next(batches), flags, at.stream), gate)
        assert e.value.kind in ("allocated", "synchronised"), e.value
    finally:
        r.close()
