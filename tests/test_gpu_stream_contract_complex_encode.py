"""-m gpu: dpfhe_encode_complex held to the stream contract (include/dpfhe.h, Conventions) behind tests/stream_gate.py's gate on a non-blocking stream:
the cases of tests/test_gpu_complex_encode.py's footprint test, every form at N = 256 (one kernel, one item) and at N = 32768 (two kernels, two items,
intermediate words parked in row 0 of each item's output), with Case.gate set as tests/test_gpu_stream_contract.py does for the older entries.

These cases live in a file of their own, collected after tests/test_gpu_stream_contract.py, on purpose.  shared_gate() picks the stream S of the whole
process the first time it is called, and which hardware queue a stream shares with which other depends on the streams alive when it is made.  The
suite so far makes S in test_gpu_stream_contract.py, after the tests that bring up torch's stream pool; asked for S before them (a file sorting at
`test_gpu_c...` did), the second stream of tests/test_gpu_stream_gate.py landed on the queue of S and its planted defect went unseen.  Here S is made
where it always was, and these cases create no stream."""
import pytest

import stream_gate as sg
import test_gpu_complex_encode as ce
import test_gpu_footprint as fp

pytestmark = pytest.mark.gpu

rig, rig32k = ce.rig, ce.rig32k


@pytest.fixture
def gated():
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    fp.Case.gate = gate
    yield gate
    fp.Case.gate = None


@pytest.mark.parametrize("log2n,items", ce.ARENA_SHAPES)
def test_stream_contract(rig, rig32k, gated, log2n, items):
    before = gated.cases
    ce.arena_cases(rig("mixed", 8) if log2n == 8 else rig32k("fold", 15), log2n, items)
    assert gated.cases == before + 5      # the five forms each went through run_gated
