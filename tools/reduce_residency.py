"""Does the shard-local reduce DISPLACE workgroups of the fused multiply while it runs beside it?  (tool; DESIGN.md section 5, "placement of the
shard-local reduce")

Runs the traced quad multiply (dpfhe_debug_ct_mul_trace: per workgroup, start / end stamps of the 100 MHz realtime clock and HW_ID | XCC_ID)
over `pairs` ciphertext pairs at N = 4096 / L = 4, once ALONE and once with dpfhe_reduce_sum of an `items` x 3 buffer running on a second stream.
The reduce kernels carry no stamps: on its stream the reduce sits between two one-pair traced multiplies, whose stamps give the window it ran in,
on the same clock (the closing marker needs a free multiply slot, so the window's end reads late by up to one workgroup lifetime).
Printed, for the multiply's steady part (10 % .. 90 % of its span) inside and outside that window:
  * multiply workgroups resident per CU (mean over the CUs seen and over 400 sample times) and the share of (CU, time) samples with 0 / 1 / 2 residents;
  * the median lifetime of the workgroups whose midpoint falls there.
usage: [DPFHE_AB_LIB=other/libdpfhe_hip.so] [TAG=name] python tools/reduce_residency.py [pairs=2048] [items=8192]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeppowers_amd import _cabi  # noqa: E402

if os.environ.get("DPFHE_AB_LIB"):
    _cabi.LIB_PATH = os.path.abspath(os.environ["DPFHE_AB_LIB"])
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator  # noqa: E402
from deeppowers_amd.params import FheParams  # noqa: E402

TW = 12   # trace words per workgroup (kernels.h kTraceWords): 0 start, 6 stores drained, 7 HW_ID | XCC_ID << 32


def records(trace):
    tr = trace.cpu().numpy().view(np.uint64).reshape(-1, TW)
    hw = tr[:, 7]
    cu = ((hw >> np.uint64(8)) & np.uint64(0xff)).astype(np.int64) | (((hw >> np.uint64(32)) & np.uint64(0xf)).astype(np.int64) << 8)
    return tr[:, 0].astype(np.int64), tr[:, 6].astype(np.int64), cu


def analyse(label, start, end, cu, window):
    """window: (t0, t1) ticks in which the reduce ran, or None"""
    t0 = start.min()
    us = lambda x: (x - t0) / 100.0
    s, e = us(start), us(end)
    span = e.max()
    keys, cu_idx = np.unique(cu, return_inverse=True)
    pts = np.linspace(0.1 * span, 0.9 * span, 400)
    alive = np.zeros((len(pts), len(keys)), dtype=np.int64)
    for i, x in enumerate(pts):
        alive[i] = np.bincount(cu_idx[(s <= x) & (e > x)], minlength=len(keys))
    mid, life = 0.5 * (s + e), e - s
    steady = (mid > 0.1 * span) & (mid < 0.9 * span)
    print(f"{label}: {len(s)} workgroups on {len(keys)} CUs, span {span:.1f} us" + (f", reduce window {us(window[0]):.1f} .. {us(window[1]):.1f} us" if window else ""))
    if window:
        w0, w1 = us(window[0]), us(window[1])
        sel = {"while the reduce runs": (pts >= w0) & (pts <= w1), "while it does not": (pts < w0) | (pts > w1)}
        wg = {"while the reduce runs": steady & (mid >= w0) & (mid <= w1), "while it does not": steady & ((mid < w0) | (mid > w1))}
    else:
        sel, wg = {"alone": np.ones(len(pts), bool)}, {"alone": steady}
    for k in sel:
        a = alive[sel[k]]
        if a.size == 0:
            print(f"  {k:22s}: no sample of the steady part falls there")
            continue
        share = [float((a == r).mean()) for r in (0, 1, 2)]
        lt = life[wg[k]]
        print(f"  {k:22s}: {a.mean():.3f} multiply workgroups resident per CU ({int(sel[k].sum())} sample times; 0 / 1 / 2 residents on "
              f"{100 * share[0]:.1f} / {100 * share[1]:.1f} / {100 * share[2]:.1f} % of the CU-samples, more on {100 * float((a > 2).mean()):.1f} %); "
              f"median lifetime {np.median(lt) if lt.size else float('nan'):.1f} us over {lt.size} workgroups")


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    items = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    p = FheParams.n4096_l4()
    ctx = Context(p, 0)
    ev = Evaluator(ctx)
    lib, L, N, dev = ctx._lib, p.n_limbs, p.n, ctx.device
    g = torch.Generator(device=dev).manual_seed(3)
    q = torch.tensor(p.moduli, dtype=torch.int64, device=dev).view(1, 1, L, 1)
    a = torch.randint(0, 2**62, (pairs, 2, L, N), generator=g, dtype=torch.int64, device=dev) % q
    b = torch.randint(0, 2**62, (pairs, 2, L, N), generator=g, dtype=torch.int64, device=dev) % q
    o = ctx.empty(pairs, components=3)
    terms = torch.randint(0, 2**62, (items, 3, L, N), generator=g, dtype=torch.int64, device=dev) % q
    total = ctx.empty(components=3)
    mo = [ctx.empty(1, components=3) for _ in range(2)]
    trace = torch.zeros(pairs * L * TW, dtype=torch.int64, device=dev)
    marks = [torch.zeros(L * TW, dtype=torch.int64, device=dev) for _ in range(2)]
    main_s, side = torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)

    def traced(out, n, tr, stream):
        _cabi.check(lib.dpfhe_debug_ct_mul_trace(ctx.handle, out.data_ptr(), a.data_ptr(), b.data_ptr(), n, tr.data_ptr(), stream.cuda_stream), "trace")

    def beside():
        side.wait_stream(main_s)
        with torch.cuda.stream(side):
            traced(mo[0], 1, marks[0], side)
            ev.reduce_sum(Ciphertext(terms), out=total, stream=side)
            traced(mo[1], 1, marks[1], side)
        traced(o, pairs, trace, main_s)
        main_s.wait_stream(side)
        torch.cuda.synchronize()

    def alone():
        traced(o, pairs, trace, main_s)
        torch.cuda.synchronize()

    for _ in range(3):   # warm chip, warm code objects
        alone(); beside()
    print(f"# tools/reduce_residency.py {os.environ.get('TAG', '')}: library {os.path.relpath(_cabi.LIB_PATH)}; {pairs} pairs traced, reduce of {items} x 3 x {L} x {N} words")
    for rep in range(2):
        alone()
        analyse(f"run {rep}, multiply alone", *records(trace), None)
        beside()
        m0, m1 = records(marks[0]), records(marks[1])
        analyse(f"run {rep}, reduce beside it", *records(trace), (int(m0[1].max()), int(m1[0].min())))
    ctx.close()


if __name__ == "__main__":
    main()
