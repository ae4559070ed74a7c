"""-m gpu: dpfhe_relinearize_lincomb_rescale_hybrid held to the stream contract (include/dpfhe.h, Conventions) behind tests/stream_gate.py's gate on a
non-blocking stream: the cases of tests/test_gpu_relin_lincomb.py's footprint test (K = 0, 2 and 5, batches 1 and 3, d_work at exactly its size, the term
pointers handed over in host arrays that are gone when the gate opens), with Case.gate set as tests/test_gpu_stream_contract.py does for the older entries.

A file of its own, collected after tests/test_gpu_stream_contract.py, for the reason tests/test_gpu_stream_contract_complex_encode.py gives: the
process's gated stream S is made where it always was, and these cases create no stream."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_relin_lincomb as tl

pytestmark = pytest.mark.gpu

rig = tl.rig


@pytest.fixture
def gated():
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    fp.Case.gate = gate
    yield gate
    fp.Case.gate = None


def test_stream_contract(rig, gated):
    before = gated.cases
    for name, log2n in tl.ARENA:
        tl.arena_cases(rig(name, log2n))
    assert gated.cases == before + 3 * len(tl.ARENA)      # every case went through run_gated
