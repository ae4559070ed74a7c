"""Slot encoding on the MI355X: dpfhe_encode_slots rate (tool).

    python tools/encode_bench.py run --out DIR      # GPU: event-timed encodes (each pass >= 0.25 s of calls) -> DIR/run.json and a text table on stdout
    rocprofv3 --kernel-trace --stats -d DIR/prof -o encode -- python tools/encode_bench.py run --min-seconds 0.02 --passes 2 --out DIR/prof_run    # kernel time, a run of its own

Workloads: the 1024 diagonals of a 768 -> 3072 layer at N = 8192 over six limbs (403 MB out) and 256 vectors at N = 16384 over six limbs, each in the
residue form (flags 0: the encode kernel alone) and the transformed form (DPFHE_ENCODE_NTT: encode + the context's forward transform in place).
Traffic counted = 4 bytes read + 8 L bytes written per coefficient (+ 16 L for the in-place transform of the NTT form); the rate is that traffic over
the event time, reported as a share of the 8 TB/s HBM peak of the MI355X - a traffic-over-time figure, not a counter reading."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("n8192_l6_ffn_up", 13, 6, 1024), ("n16384_l6", 14, 6, 256))   # (name, log2 N, L, items)
HBM_PEAK = 8.0e12
T_MOD = 65537


def run(args):
    import numpy as np
    import torch

    from deeppowers_amd import _cabi
    from deeppowers_amd.evaluator import Context
    from deeppowers_amd.params import FheParams, ntt_primes
    rows = []
    for name, log2n, limbs, items in SHAPES:
        p = FheParams.n8192_l6() if (log2n, limbs) == (13, 6) else ntt_primes(log2n, limbs)
        ctx = Context(p, 0)
        enc = ctx.encoder(T_MOD)
        rng = np.random.default_rng(1)
        slots = torch.from_numpy(rng.integers(0, T_MOD, (items, p.n), dtype=np.int64).astype(np.int32)).to(ctx.device)
        out = torch.empty((items, limbs, p.n), dtype=torch.int64, device=ctx.device)
        stream = torch.cuda.current_stream(ctx.device).cuda_stream
        for form, flags in (("residues", 0), ("ntt", _cabi.ENCODE_NTT)):
            call = lambda: _cabi.check(ctx._lib.dpfhe_encode_slots(enc, out.data_ptr(), slots.data_ptr(), items, flags, stream), "dpfhe_encode_slots")
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
            coeffs = items * p.n
            traffic = coeffs * (4 + 8 * limbs + (16 * limbs if flags else 0))
            best, med = min(passes), sorted(passes)[len(passes) // 2]
            rows.append({"shape": name, "form": form, "items": items, "log2_n": log2n, "limbs": limbs, "bytes_out": coeffs * 8 * limbs, "traffic_bytes": traffic,
                         "reps": reps, "pass_seconds_per_call": passes, "us_per_call_median": med * 1e6, "us_per_call_best": best * 1e6,
                         "timed_seconds_per_pass": med * reps, "tb_per_s_median": traffic / med / 1e12, "share_of_hbm_peak_median": traffic / med / HBM_PEAK})
        ctx.close()
    os.makedirs(args.out, exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "t": T_MOD, "rows": rows}, open(os.path.join(args.out, "run.json"), "w"), indent=1)
    print(f"dpfhe_encode_slots on {torch.cuda.get_device_name(0)}: device events around >= {args.min_seconds} s of calls, {args.passes} passes, median pass")
    print(f"{'shape':18} {'form':9} {'items':>6} {'MB out':>8} {'us/call':>10} {'TB/s (traffic/time)':>20} {'share of 8 TB/s':>16} {'s timed/pass':>13}")
    for r in rows:
        print(f"{r['shape']:18} {r['form']:9} {r['items']:6d} {r['bytes_out'] / 1e6:8.1f} {r['us_per_call_median']:10.1f} {r['tb_per_s_median']:20.3f} "
              f"{100 * r['share_of_hbm_peak_median']:15.1f}% {r['timed_seconds_per_pass']:13.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--reps", type=int, default=40)
    r.add_argument("--min-seconds", type=float, default=0.25, help="each timed pass repeats the call until it fills this long")
    r.add_argument("--passes", type=int, default=5)
    r.add_argument("--warmup", type=int, default=3)
    r.add_argument("--out", required=True)
    r.set_defaults(fn=run)
    args = ap.parse_args()
    args.fn(args)


if __name__ == "__main__":
    main()
