"""-m gpu: dpfhe_rotate_matvec_hoisted_qp behind tests/stream_gate.py's gate: the footprint case of tests/test_gpu_rotate_matvec.py at N = 4096 and at
N = 16384 (arena scratch, sized by the warm-up).  Its own file, collected after tests/test_gpu_stream_contract.py:
tests/test_gpu_stream_contract_complex_encode.py gives the reason."""
import pytest

import stream_gate as sg
import test_gpu_footprint as fp
import test_gpu_rotate_matvec as trm

pytestmark = pytest.mark.gpu
rig = trm.rig


def test_stream_contract(rig):
    gate = sg.shared_gate("cuda:0")      # raises unless its planted defects were reported
    before, fp.Case.gate = gate.cases, gate
    try:
        for log2n in (12, 14):
            trm.arena_cases(rig("fold", log2n, 3))
    finally:
        fp.Case.gate = None
    assert gate.cases == before + 2      # every case went through run_gated
