"""-m gpu: dpfhe_rotate_add_hybrid held to the stream contract (include/dpfhe.h, Conventions) behind tests/stream_gate.py's gate on a non-blocking stream: the
cases of tests/test_gpu_rotate_add.py's footprint test (1 and 3 steps of 1 and 3 items on the fused key switch, d_acc NULL at one step; two shapes on the
composed key products, whose arena scratch has its size after the gate's warm-up run), with Case.gate set as tests/test_gpu_stream_contract.py does for
the older entries.

A file of its own, collected after tests/test_gpu_stream_contract.py, for the reason tests/test_gpu_stream_contract_complex_encode.py gives: the
process's gated stream S is made where it always was, and these cases create no stream."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_rotate_add as tra

pytestmark = pytest.mark.gpu

rig = tra.rig


@pytest.fixture
def gated():
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    fp.Case.gate = gate
    yield gate
    fp.Case.gate = None


def test_stream_contract(rig, gated):
    before = gated.cases
    for name, log2n, shapes in tra.FOOTPRINT:
        tra.arena_cases(rig(name, log2n), shapes)
    assert gated.cases == before + sum(len(shapes) for _, _, shapes in tra.FOOTPRINT) == before + 10      # every case went through run_gated
