"""-m gpu: dpfhe_relinearize_rescale_hybrid and dpfhe_lincomb_rescale held to the stream contract (include/dpfhe.h, Conventions) behind tests/stream_gate.py's
gate on a non-blocking stream: the cases of tests/test_gpu_fused_rescale.py's footprint test (batches 1 and 3 of the relinearisation with d_work at exactly its
size, K = 3 and K = 16 of the linear combination), with Case.gate set as tests/test_gpu_stream_contract.py does for the older entries.

A file of its own, collected after tests/test_gpu_stream_contract.py, for the reason tests/test_gpu_stream_contract_complex_encode.py gives: the
process's gated stream S is made where it always was, and these cases create no stream."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_fused_rescale as fu

pytestmark = pytest.mark.gpu

rig = fu.rig


@pytest.fixture
def gated():
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    fp.Case.gate = gate
    yield gate
    fp.Case.gate = None


def test_stream_contract(rig, gated):
    before = gated.cases
    fu.arena_cases(rig("pinned_ld4", 8))
    fu.arena_cases(rig("f64_under_fold", 12))
    assert gated.cases == before + 8      # every case went through run_gated
