"""CPU: every rejection of dpfhe_ct_mul_outer that the arguments alone decide returns 2000 with no device and no context (the entry makes them before it
looks at the context); the two that need the ring's size - the output overlapping an operand, a_items * b_items too large - come before the device is touched
all the same (source order here, the calls themselves in tests/test_gpu_mul_outer.py).  The Python mirror is there, and the header's prose names every
rejection the implementation makes."""
import ctypes as C
import os
import re

import pytest

from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = _cabi.OUTER_CAUSAL


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_cabi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _cabi.load()


@pytest.fixture(scope="module")
def bufs():
    """host memory, 16-byte aligned: the entry must not read it, let alone hand it to a device"""
    raw = (C.c_uint64 * 64)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, base, base + 128, base + 256


def test_flag_bits():
    assert CAUSAL == 4 and CAUSAL & (_cabi.IN_NTT | _cabi.OUT_NTT) == 0


def test_rejections_that_need_no_context(lib, bufs):
    _, out, a, b = bufs
    f, err = lib.dpfhe_ct_mul_outer, lib.dpfhe_last_error
    assert f(None, out, a, b, 2, 3, 0, None) == 2000 and b"dpfhe_ct_mul_outer" in err() and b"null context" in err()      # nothing else wrong
    for flags in (8, 16, 1 << 31, 7 | 8):
        assert f(None, out, a, b, 2, 2, flags, None) == 2000 and b"unknown flag" in err(), flags
    for flags in (CAUSAL, CAUSAL | _cabi.IN_NTT | _cabi.OUT_NTT):
        assert f(None, out, a, b, 2, 3, flags, None) == 2000 and b"causal" in err()
        assert f(None, out, a, b, 3, 3, flags, None) == 2000 and b"null context" in err()                                     # equal counts pass that check
    for args in ((None, a, b), (out, None, b), (out, a, None), (out + 8, a, b), (out, a + 8, b), (out, a, b + 8)):
        assert f(None, *args, 2, 3, 0, None) == 2000 and b"null or misaligned" in err(), args
    for A, B in ((1 << 31, 1), (1, 1 << 31), (1 << 63, 1 << 63)):
        assert f(None, out, a, b, A, B, 0, None) == 2000 and b"too large" in err(), (A, B)
    assert f(None, None, None, None, 0, 5, 0, None) == 2000 and b"null context" in err()                                      # nothing to do, but no context either


def test_python_mirror_exists():
    assert callable(Evaluator.multiply_outer)


def entry_source():
    src = open(os.path.join(ROOT, "deeppowers_amd", "csrc", "cabi_mul.hip")).read()
    start = src.index('extern "C" int dpfhe_ct_mul_outer(')
    return src[start:src.index("\n}\n", start)]


def header_prose():
    hdr = open(os.path.join(ROOT, "include", "dpfhe.h")).read()
    end = hdr.index("int dpfhe_ct_mul_outer(")
    return " ".join(re.sub(r"\n \* ?", "\n", hdr[hdr.rindex("/*", 0, end):end]).split())      # without the comment's line leaders


def test_header_names_every_rejection_the_entry_makes():
    body, prose = entry_source(), header_prose()
    details = re.findall(r'fail\(DPFHE_INVALID_ARGUMENT, what, "([^"]+)"\)', body)
    assert len(details) == len(re.findall(r"\bfail\(", body)) == 7          # every early return of the entry is an INVALID_ARGUMENT with a detail
    rejections = prose[prose.index("DPFHE_INVALID_ARGUMENT, before the device is touched"):]
    named = {"null context": None,                                             # the ABI-wide rule: not restated per entry
             "unknown flag": "an unknown flag",
             "the causal form needs a_items == b_items": "DPFHE_OUTER_CAUSAL with a_items != b_items",
             "null or misaligned buffer": "a null or misaligned (16 bytes) buffer",
             "a_items * b_items too large for one launch": "a_items * b_items too large for one launch",      # (twice: the counts alone, then with the ring's size)
             "output overlaps an operand": "d_out3 overlapping an operand"}
    assert sorted(set(details)) == sorted(named) and details.count("a_items * b_items too large for one launch") == 2
    for detail, words in named.items():
        assert words is None or words in rejections, detail
    assert "a_items == 0 or b_items == 0 returns success" in rejections
    assert body.index("DPFHE_ON_DEVICE") > max(body.rindex(d) for d in details)      # all of them before the device is touched
    # the sizes are tested before the products that could wrap, and before the overlap test that multiplies them
    assert body.index("a_items > kMaxGrid || b_items > kMaxGrid") < body.index("a_items * b_items > kMaxGrid") < body.index("overlaps(")
    # ... and the rest the issue asks of the prose: layouts, aliasing, scratch, traffic
    assert "d_out3[i * b_items + j] = a[i] (x) b[j]" in prose and "d_out3[i (i + 1) / 2 + j] = a[i] (x) b[j] for j <= i" in prose
    assert "may alias each other" in prose and "d_out3 must not overlap either operand" in prose
    assert "With DPFHE_IN_NTT there is no scratch at all" in prose and "6 items at least" in prose and "a limit below that is EXCEEDED, to exactly 6 items" in prose
    assert "2 a_items + 2 b_items ceil(a_items / 4) read, 3 per pair written" in prose


def test_neither_instantiation_of_the_kernel_uses_scratch_memory(lib):
    """tests/test_cabi_cpu.py lets a generic-prime kernel keep a few words in scratch memory; this one is documented at ScratchSize 0 on both policies (a rolled
    loop over a block's keys kept the key buffers there: 144 bytes per lane), and at the VGPR counts DESIGN.md states"""
    log = os.path.join(ROOT, "deeppowers_amd", "csrc", "build", "cabi_mul.log")
    if not os.path.exists(log):
        pytest.skip("no build log (library was not built in this checkout)")
    seen = {}
    for block in open(log).read().split("Function Name: ")[1:]:
        name = block.split("\n")[0]
        if "tensor3_outer_kernel" in name:
            policy = "FoldArith" if "FoldArith" in name else "ShoupArith" if "ShoupArith" in name else name
            seen[policy] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)), int(re.search(r" VGPRs: (\d+)", block).group(1)))
    assert set(seen) == {"FoldArith", "ShoupArith"} and all(s == 0 for s, _ in seen.values()), seen
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"{seen['FoldArith'][1]}/{seen['ShoupArith'][1]} VGPRs" in design, seen
    assert seen["FoldArith"][1] <= 128          # two 256-thread workgroups and more per CU: 512 VGPRs per SIMD lane, 4 waves of 128
