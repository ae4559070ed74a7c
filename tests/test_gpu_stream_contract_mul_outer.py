"""-m gpu: dpfhe_ct_mul_outer held to the stream contract (include/dpfhe.h, Conventions) behind tests/stream_gate.py's gate on a non-blocking stream: the cases
of tests/test_gpu_mul_outer.py's footprint test (full and causal and with aliased operands through the stream's scratch arena, which the warm-up call has
grown; the NTT-domain forms that take none), with Case.gate set as tests/test_gpu_stream_contract.py does for the older entries.

A file of its own, collected after tests/test_gpu_stream_contract.py, for the reason tests/test_gpu_stream_contract_complex_encode.py gives: the
process's gated stream S is made where it always was, and these cases create no stream."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_mul_outer as tm

pytestmark = pytest.mark.gpu

rig = tm.rig


@pytest.fixture
def gated():
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    fp.Case.gate = gate
    yield gate
    fp.Case.gate = None


def test_stream_contract(rig, gated):
    before = gated.cases
    for name, log2n in tm.ARENA:
        tm.arena_cases(rig(name, log2n))
    assert gated.cases == before + tm.ARENA_CASES * len(tm.ARENA)      # every case went through run_gated
