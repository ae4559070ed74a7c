"""Complex slot encoding on the MI355X: dpfhe_encode_complex rate (tool).

    python tools/cencode_bench.py run --out DIR      # GPU: event-timed encodes (each pass >= 0.25 s of calls) -> DIR/run.json and a text table on stdout
    python tools/cencode_bench.py host               # no GPU: seconds per vector of the host twin (dpfhe_encode_complex_host)

Workload: 1024 slot vectors at N = 8192 over six limbs (the shape of tools/encode_bench.py's first row), in the residue form (flags 0: the encode kernel
alone) and the transformed form (DPFHE_ENCODE_NTT: encode + the context's forward transform in place).  Algorithmic traffic = 8 N bytes read + 8 L N
written per vector (the NTT form's in-place transform is not counted: the figure is the encoder's share of a roofline, so the NTT form reads lower by
construction); the rate is that traffic over the event time, reported as a share of the 8 TB/s HBM peak - a traffic-over-time figure, not a counter
reading."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG2N, LIMBS, ITEMS = 13, 6, 1024
HBM_PEAK = 8.0e12
SCALE = 2.0 ** 40


def run(args):
    import numpy as np
    import torch

    from deeppowers_amd import _cabi
    from deeppowers_amd.evaluator import Context
    from deeppowers_amd.params import FheParams
    p = FheParams.n8192_l6()
    ctx = Context(p, 0)
    enc = ctx.complex_encoder()
    rng = np.random.default_rng(1)
    slots = torch.from_numpy(rng.uniform(-1, 1, (ITEMS, p.n // 2)) + 1j * rng.uniform(-1, 1, (ITEMS, p.n // 2))).to(ctx.device)
    out = torch.empty((ITEMS, LIMBS, p.n), dtype=torch.int64, device=ctx.device)
    stream = torch.cuda.current_stream(ctx.device).cuda_stream
    rows = []
    for form, flags in (("residues", 0), ("ntt", _cabi.ENCODE_NTT)):
        call = lambda: _cabi.check(ctx._lib.dpfhe_encode_complex(enc, out.data_ptr(), slots.data_ptr(), ITEMS, SCALE, flags, stream), "dpfhe_encode_complex")
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            call()
        e1.record()
        torch.cuda.synchronize()
        reps = max(args.reps, int(args.min_seconds / (e0.elapsed_time(e1) * 1e-3 / 8)) + 1)   # a timed pass fills min_seconds
        passes = []
        for _ in range(args.passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            passes.append(e0.elapsed_time(e1) * 1e-3 / reps)
        traffic = ITEMS * (8 * p.n + 8 * LIMBS * p.n)
        med = sorted(passes)[len(passes) // 2]
        rows.append({"form": form, "items": ITEMS, "log2_n": LOG2N, "limbs": LIMBS, "traffic_bytes": traffic, "reps": reps, "pass_seconds_per_call": passes,
                     "us_per_call_median": med * 1e6, "us_per_call_min": min(passes) * 1e6, "us_per_call_max": max(passes) * 1e6,
                     "tb_per_s_median": traffic / med / 1e12, "share_of_hbm_peak_median": traffic / med / HBM_PEAK})
    ctx.close()
    os.makedirs(args.out, exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, open(os.path.join(args.out, "run.json"), "w"), indent=1)
    print(f"dpfhe_encode_complex on {torch.cuda.get_device_name(0)}: {ITEMS} vectors, N = {p.n}, L = {LIMBS}; device events around >= {args.min_seconds} s of "
          f"calls, {args.passes} passes")
    print(f"{'form':9} {'us/call median':>15} {'min':>9} {'max':>9} {'TB/s (traffic/time)':>20} {'share of 8 TB/s':>16} {'reps/pass':>10}")
    for r in rows:
        print(f"{r['form']:9} {r['us_per_call_median']:15.1f} {r['us_per_call_min']:9.1f} {r['us_per_call_max']:9.1f} {r['tb_per_s_median']:20.3f} "
              f"{100 * r['share_of_hbm_peak_median']:15.1f}% {r['reps']:10d}")


def host(args):
    import numpy as np

    from deeppowers_amd import ckks
    from deeppowers_amd.params import FheParams
    p = FheParams.n8192_l6()
    rng = np.random.default_rng(1)
    z = rng.uniform(-1, 1, (args.items, p.n // 2)) + 1j * rng.uniform(-1, 1, (args.items, p.n // 2))
    ckks.encode_host(z, SCALE, LOG2N, p.moduli)
    times = []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        ckks.encode_host(z, SCALE, LOG2N, p.moduli)
        times.append((time.perf_counter() - t0) / args.items)
    print(f"dpfhe_encode_complex_host, N = {p.n}, L = {LIMBS}, {args.items} vectors per call (tables rebuilt per call): median {sorted(times)[len(times) // 2] * 1e6:.0f} us "
          f"per vector (min {min(times) * 1e6:.0f}, max {max(times) * 1e6:.0f}, {args.passes} passes)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--reps", type=int, default=40)
    r.add_argument("--min-seconds", type=float, default=0.25, help="each timed pass repeats the call until it fills this long")
    r.add_argument("--passes", type=int, default=7)
    r.add_argument("--warmup", type=int, default=3)
    r.add_argument("--out", required=True)
    r.set_defaults(fn=run)
    h = sub.add_parser("host")
    h.add_argument("--items", type=int, default=64)
    h.add_argument("--passes", type=int, default=5)
    h.set_defaults(fn=host)
    args = ap.parse_args()
    args.fn(args)


if __name__ == "__main__":
    main()
