"""-m gpu: dpfhe_switch_key_grouped behind tests/stream_gate.py's gate: the footprint cases of tests/test_gpu_switch_key_grouped.py at N = 256 and N = 16384 (composed
transforms, arena scratch sized by the warm-up, which also uploads the digit-group table).  Its own file, collected after tests/test_gpu_stream_contract.py:
tests/test_gpu_stream_contract_complex_encode.py gives the reason."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_switch_key_grouped as tsk

pytestmark = pytest.mark.gpu
cases = tsk.cases


def test_stream_contract(cases):
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    before, fp.Case.gate = gate.cases, gate
    try:
        for shape in tsk.FOOTPRINT:
            tsk.arena_cases(cases(*shape))
    finally:
        fp.Case.gate = None
    assert gate.cases == before + 4      # every case went through run_gated
