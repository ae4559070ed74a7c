"""CPU: the register arithmetic that lets the shard-local reduce run BESIDE the fused multiply, read from the build logs.
Two workgroups of ct_mul_quad_kernel<FoldArith, 12, 4> hold 2 x 240 of a SIMD lane's 512 registers; reduce_thin_kernel lives in the 32 that are
left, without scratch and without LDS.  A compiler or source change that breaks either budget would silently put the reduce back in the
multiply's place: this test makes it loud."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD = "ct_mul_quad_kernelINS_9FoldArithELi12ELi4ELb0ELb0E"   # ct_mul_quad_kernel<FoldArith, 12, 4, false, false>, mangled
THIN = "reduce_thin_kernelE"


def _usage():
    """{mangled kernel name: [(VGPRs + AGPRs, scratch bytes per lane, LDS bytes per block), ...]} over all build logs"""
    out = {}
    for path in glob.glob(os.path.join(ROOT, "deeppowers_amd", "csrc", "build", "*.log")):
        for block in open(path).read().split("Function Name: ")[1:]:
            def field(key):
                m = re.search(re.escape(key) + r": (\d+)", block)
                return int(m.group(1)) if m else None
            v, a, s, l = field(" VGPRs"), field(" AGPRs"), field("ScratchSize [bytes/lane]"), field("LDS Size [bytes/block]")
            if v is not None:
                out.setdefault(block.split()[0], []).append((v + (a or 0), s, l))
    return out


def test_the_reduce_fits_the_registers_the_multiply_leaves():
    usage = _usage()
    if not usage:
        pytest.skip("no build logs (library was not built in this checkout)")
    quad = [u for name, us in usage.items() if QUAD in name for u in us]
    thin = [u for name, us in usage.items() if THIN in name for u in us]
    assert quad, "ct_mul_quad_kernel<FoldArith, 12, 4, false, false> is missing from the build logs"
    assert thin, "reduce_thin_kernel is missing from the build logs"
    for regs, scratch, _ in quad:
        assert regs <= 240, f"the quad multiply holds {regs} registers: two workgroups leave fewer than 32 of 512"
        assert scratch == 0
    for regs, scratch, lds in thin:
        assert regs <= 32, f"reduce_thin_kernel needs {regs} registers: it no longer fits beside two multiply workgroups"
        assert scratch == 0, f"reduce_thin_kernel spills {scratch} bytes per lane"
        assert lds == 0, "reduce_thin_kernel must not take LDS from the multiply"
