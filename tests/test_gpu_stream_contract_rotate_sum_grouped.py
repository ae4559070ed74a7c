"""-m gpu: dpfhe_rotate_sum_hoisted_grouped behind tests/stream_gate.py's gate: the footprint cases of tests/test_gpu_rotate_sum_grouped.py at N = 256 and N = 16384
(composed transforms, arena scratch).  The rig's constructor makes the warm-up call, so the digit-group table is on the device before the gate closes.  Its own
file, collected after tests/test_gpu_stream_contract.py: tests/test_gpu_stream_contract_complex_encode.py gives the reason."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_rotate_sum_grouped as trs

pytestmark = pytest.mark.gpu
rigs = trs.rigs


def test_stream_contract(rigs):
    made = [rigs(*shape) for shape in trs.FOOTPRINT]      # (warmed up)
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    before, fp.Case.gate = gate.cases, gate
    try:
        for r in made:
            trs.arena_cases(r)
    finally:
        fp.Case.gate = None
    assert gate.cases == before + 4      # every case went through run_gated
