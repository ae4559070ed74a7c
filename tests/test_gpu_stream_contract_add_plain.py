"""-m gpu: dpfhe_add_plain held to the stream contract (include/dpfhe.h, Conventions) behind tests/stream_gate.py's gate on a non-blocking stream: the
two cases of tests/test_gpu_add_plain.py's footprint test (out of place and in place, on the all-class mixture at N = 256), with Case.gate set as
tests/test_gpu_stream_contract.py does for the older entries.

A file of its own, collected after tests/test_gpu_stream_contract.py, for the reason tests/test_gpu_stream_contract_complex_encode.py gives: the
process's gated stream S is made where it always was, and these cases create no stream."""
import pytest

import stream_gate as sg
import test_gpu_add_plain as ap
import test_gpu_footprint as fp

pytestmark = pytest.mark.gpu

rig = ap.rig


@pytest.fixture
def gated():
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    fp.Case.gate = gate
    yield gate
    fp.Case.gate = None


def test_stream_contract(rig, gated):
    before = gated.cases
    ap.arena_cases(rig("mixed", 8))
    assert gated.cases == before + 2      # both cases went through run_gated
