"""CPU: dpfhe_ct_mul_complement refuses a null context before it looks at anything else (no compute calls here: no GPU), the Python mirror is there, and the
header's prose for the entry names every rejection the implementation makes."""
import os
import re

import pytest

from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_cabi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _cabi.load()


def test_null_context_is_rejected(lib):
    assert lib.dpfhe_ct_mul_complement(None, None, None, None, None, 1, 1, 1, 0, None) == 2000
    assert b"dpfhe_ct_mul_complement" in lib.dpfhe_last_error() and b"null context" in lib.dpfhe_last_error()
    assert lib.dpfhe_ct_mul_complement(None, None, None, None, None, 0, 0, 0, 7, None) == 2000      # ... whatever else is wrong, or nothing


def test_python_mirror_exists():
    assert callable(Evaluator.multiply_complement)


def entry_source():
    src = open(os.path.join(ROOT, "deeppowers_amd", "csrc", "cabi_mul.hip")).read()
    start = src.index('extern "C" int dpfhe_ct_mul_complement(')
    return src[start:src.index("\n}\n", start)]


def header_prose():
    hdr = open(os.path.join(ROOT, "include", "dpfhe.h")).read()
    end = hdr.index("int dpfhe_ct_mul_complement(")
    return " ".join(re.sub(r"\n \* ?", "\n", hdr[hdr.rindex("/*", 0, end):end]).split())      # without the comment's line leaders


def test_header_names_every_rejection_the_entry_makes():
    body, prose = entry_source(), header_prose()
    details = re.findall(r'fail\(DPFHE_INVALID_ARGUMENT, what, "([^"]+)"\)', body)
    assert len(details) == len(re.findall(r"\bfail\(", body)) == 6          # every early return of the entry is an INVALID_ARGUMENT with a detail
    rejections = prose[prose.index("DPFHE_INVALID_ARGUMENT, before the device is touched"):]
    named = {"null context": None,                                             # the ABI-wide rule: not restated per entry
             "unknown flag": "an unknown flag",
             "terms must be at least 1 when there is no self product": "terms == 0 without with_self",
             "null or misaligned buffer": "a null or misaligned (16 bytes) buffer",
             "groups * (terms + 1) too large for one launch": "groups * (terms + 1) too large for one launch",
             "output overlaps an operand": "d_out3 overlapping an operand or d_kappa"}
    assert sorted(details) == sorted(named)
    for detail, words in named.items():
        assert words is None or words in rejections, detail
    assert "groups == 0 returns success" in rejections
    assert body.index("DPFHE_ON_DEVICE") > max(body.index(d) for d in details)      # all of them before the device is touched
    # ... and the rest the issue asks of the prose: aliasing, traffic
    assert "may alias each other" in prose and "must overlap none of d_a2, d_b2, d_kappa" in prose
    assert "2 terms + 2 read, 3 (terms + with_self) written" in prose
