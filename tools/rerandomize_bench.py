"""Noise sampling and re-randomisation on the MI355X: rates of dpfhe_sample_noise next to dpfhe_expand_uniform, and the cost of
dpfhe_rerandomize next to the layer it protects (tool).

    python tools/rerandomize_bench.py run --out DIR      # GPU: event-timed calls (each pass >= 0.25 s of calls) -> DIR/run.json and a text table on stdout
    rocprofv3 --kernel-trace --stats -d DIR/prof -o noise -- python tools/rerandomize_bench.py run --min-seconds 0.02 --passes 2 --skip-layer --out DIR/prof_run

(i) N = 8192, L = 5 (the data limbs of the packed layers), 64 items (21 MB: launch-bound) and 2048 items (671 MB: beyond the Infinity Cache) of one
    component per call: dpfhe_sample_noise for each kind (flood at 100 and at
    200 bits: one or two 128-bit reductions per coefficient) and dpfhe_expand_uniform of the same build in the same run.  Rates are coefficients
    (one per limb row: N L items words) per second and bytes written per second, read against the 8 TB/s HBM peak - traffic over time, not a counter.
(ii) examples/encrypted_rerandomize as a child process under its own time limit: the 768 x 768 layer's apply and dpfhe_rerandomize of its 8-token
    output, medians of the same run."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
ITEMS = (64, 2048)


def timed(call, torch, args):
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
    return reps, passes


def run(args):
    import torch

    from deeppowers_amd import _cabi
    from deeppowers_amd.evaluator import Context
    from deeppowers_amd.params import FheParams
    p6 = FheParams.n8192_l6()
    p = FheParams(p6.log2_n, tuple(p6.moduli[:5]), tuple(p6.psi[:5]))
    ctx = Context(p, 0)
    lib, h = ctx._lib, ctx.handle
    seed = bytes(range(32))
    stream = torch.cuda.current_stream(ctx.device).cuda_stream
    rows = []
    for items in ITEMS:
        out = torch.zeros((items, 1, p.n_limbs, p.n), dtype=torch.int64, device=ctx.device)
        calls = [("expand_uniform", lambda: _cabi.check(lib.dpfhe_expand_uniform(h, out.data_ptr(), items, 1, 0, seed, 0, stream), "dpfhe_expand_uniform"))]
        for name, kind, param, flags in (("noise ternary", 0, 0, 0), ("noise cbd21", 1, 0, 0), ("noise flood 100", 2, 100, 0), ("noise flood 200", 2, 200, 0),
                                         ("noise flood 100 +=", 2, 100, _cabi.NOISE_ADD)):
            calls.append((name, lambda kind=kind, param=param, flags=flags: _cabi.check(
                lib.dpfhe_sample_noise(h, out.data_ptr(), items, 1, 0, kind, param, 2, seed, 0, flags, stream), "dpfhe_sample_noise")))
        words = items * p.n_limbs * p.n
        for name, call in calls:
            reps, passes = timed(call, torch, args)
            med = sorted(passes)[len(passes) // 2]
            written = words * 8
            rows.append({"call": name, "items": items, "log2_n": p.log2_n, "limbs": p.n_limbs, "reps": reps, "pass_seconds_per_call": passes,
                         "us_per_call_median": med * 1e6, "us_per_call_best": min(passes) * 1e6, "g_coefficients_per_s_median": words / med / 1e9,
                         "tb_written_per_s_median": written / med / 1e12, "share_of_hbm_peak_median": written / med / HBM_PEAK,
                         "timed_seconds_per_pass": med * reps})
        del out
    ctx.close()
    layer = None
    if not args.skip_layer:
        exe = os.path.join(ROOT, "examples", "encrypted_rerandomize")
        child = subprocess.run([exe, "8", "30"], capture_output=True, text=True, timeout=args.layer_timeout)
        layer = {"returncode": child.returncode, "stdout": child.stdout}
        for line in child.stdout.splitlines():
            if line.startswith("{"):
                layer["result"] = json.loads(line)
    os.makedirs(args.out, exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "rows": rows, "layer": layer}, open(os.path.join(args.out, "run.json"), "w"), indent=1)
    print(f"dpfhe_sample_noise / dpfhe_expand_uniform on {torch.cuda.get_device_name(0)}: N = {p.n}, L = {p.n_limbs}; device events "
          f"around >= {args.min_seconds} s of calls, {args.passes} passes, median pass")
    print(f"{'call':20} {'items':>6} {'us/call':>10} {'G coeff/s':>10} {'TB/s written':>13} {'share of 8 TB/s':>16} {'s timed/pass':>13}")
    for r in rows:
        print(f"{r['call']:20} {r['items']:6d} {r['us_per_call_median']:10.1f} {r['g_coefficients_per_s_median']:10.1f} {r['tb_written_per_s_median']:13.3f} "
              f"{100 * r['share_of_hbm_peak_median']:15.1f}% {r['timed_seconds_per_pass']:13.3f}")
    if layer is not None:
        print("examples/encrypted_rerandomize 8 30 (child process):")
        print(layer["stdout"].rstrip())
        if layer["returncode"] != 0:
            sys.exit(1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--reps", type=int, default=40)
    r.add_argument("--min-seconds", type=float, default=0.25, help="each timed pass repeats the call until it fills this long")
    r.add_argument("--passes", type=int, default=5)
    r.add_argument("--warmup", type=int, default=3)
    r.add_argument("--skip-layer", action="store_true", help="part (i) only")
    r.add_argument("--layer-timeout", type=float, default=240.0)
    r.add_argument("--out", required=True)
    r.set_defaults(fn=run)
    args = ap.parse_args()
    args.fn(args)


if __name__ == "__main__":
    main()
