"""CPU: dpfhe_ct_mul_sum refuses a null context before it looks at anything else (no compute calls here: no GPU), and the Python mirror is there."""
import pytest

from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Evaluator


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_cabi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _cabi.load()


def test_null_context_is_rejected(lib):
    assert lib.dpfhe_ct_mul_sum(None, None, None, None, 1, 1, 1, 0, None) == 2000
    assert b"dpfhe_ct_mul_sum" in lib.dpfhe_last_error() and b"null context" in lib.dpfhe_last_error()
    assert lib.dpfhe_ct_mul_sum(None, None, None, None, 0, 0, 0, 7, None) == 2000      # ... whatever else is wrong, or nothing


def test_python_mirror_exists():
    assert callable(Evaluator.multiply_sum)
