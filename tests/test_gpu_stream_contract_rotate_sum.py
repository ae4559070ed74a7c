"""-m gpu: dpfhe_rotate_sum_hoisted behind tests/stream_gate.py's gate: the footprint cases of tests/test_gpu_rotate_sum.py at N = 4096 and N = 16384 (arena scratch,
sized by the warm-up).  Its own file, collected after tests/test_gpu_stream_contract.py: tests/test_gpu_stream_contract_complex_encode.py gives the reason."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_rotate_sum as trs

pytestmark = pytest.mark.gpu
rig = trs.rig


def test_stream_contract(rig):
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    before, fp.Case.gate = gate.cases, gate
    try:
        for kind, log2n in trs.FOOTPRINT[1:]:
            trs.arena_cases(rig(kind, log2n))
    finally:
        fp.Case.gate = None
    assert gate.cases == before + 4      # every case went through run_gated
