"""Seeded uniform polynomials on the MI355X: dpfhe_expand_uniform kernel rate, and PolyBuffer::load_seeded against load (tool).

    python tools/expand_bench.py run [--reps 50] --out DIR            # GPU: event-timed expansions + the C++ load / load_seeded timing -> DIR/run.json
    rocprofv3 --kernel-trace --stats -d DIR/prof -o expand -- python tools/expand_bench.py run --reps 20 --no-load --out DIR/prof_run
    python tools/expand_bench.py report --run DIR/run.json --prof DIR/prof      # anywhere: the text committed under profiles/

Workloads (component 1 of two-component buffers, the c1 of fresh ciphertexts): 8192 items at N = 4096 / L = 4 and 512 items at N = 16384 / L = 6.
Bytes written = 8 per coefficient (the kernel reads only its limb constants).  The kernel is VALU-bound: its bound is the disassembled
instruction count of expand_uniform_kernel per lane (= per ChaCha block = 4 coefficients) over the chip's VALU issue rate, 256 CUs x 4 SIMDs
x one wave64 instruction per 2 cycles."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("n4096_l4", 12, 4, 8192), ("n16384_l6", 14, 6, 512))   # (name, log2 N, L, items)
CLOCK_GHZ, CUS, SIMDS = 2.4, 256, 4                                # MI355X: max clock, CUs, SIMDs per CU


def params_of(log2n, limbs):
    from deeppowers_amd.params import FheParams, ntt_primes
    return FheParams.n4096_l4() if (log2n, limbs) == (12, 4) else ntt_primes(log2n, limbs)


LOAD_SRC = r"""
#include <chrono>
#include <cstdio>
#include <sstream>
#include <vector>
#include "deeppowers/fhe.hpp"
using namespace deeppowers::fhe;
int main(int argc, char** argv) {
    const size_t batch = 1024; const int reps = argc > 1 ? atoi(argv[1]) : 5;
    const FheParams p = FheParams::n4096_l4();
    Context ctx(p, 0);
    KeyGenerator kg(ctx, TestSeed{1});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{2});
    std::vector<int64_t> m(batch * p.n(), 7);
    Ciphertext c(ctx, 2, batch), back(ctx, 2, batch);
    Seed seed{};
    enc.encrypt_seeded(m.data(), 40, c, seed);
    std::ostringstream o1, o2; c.save(o1); c.save_seeded(o2, seed);
    const std::string v1 = o1.str(), s1 = o2.str();
    auto t = [&](bool seeded) {
        double best = 1e30;
        for (int r = 0; r < reps + 1; ++r) {
            std::istringstream is(seeded ? s1 : v1);
            ctx.synchronize();
            auto t0 = std::chrono::steady_clock::now();
            if (seeded) back.load_seeded(is); else back.load(is);
            ctx.synchronize();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r > 0 && ms < best) best = ms;   // r = 0 warms up
        }
        return best;
    };
    const double lv1 = t(false), ls1 = t(true);
    std::printf("{\"ciphertexts\": %zu, \"v1_bytes\": %zu, \"seeded_bytes\": %zu, \"load_ms\": %.3f, \"load_seeded_ms\": %.3f, \"reps\": %d}\n",
                batch, v1.size(), s1.size(), lv1, ls1, reps);
    return 0;
}
"""


def run_load(reps):
    d = tempfile.mkdtemp()
    src, exe, lib = os.path.join(d, "load.cpp"), os.path.join(d, "load"), os.path.join(ROOT, "deeppowers_amd")
    open(src, "w").write(LOAD_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib, "-ldpfhe_api", "-ldpfhe_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(reps)], capture_output=True, text=True, timeout=600, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def run(args):
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator
    assert torch.cuda.is_available(), "expand_bench run needs a GPU"
    res = {"shapes": []}
    seed = bytes(range(32))
    for name, log2n, limbs, items in SHAPES:
        p = params_of(log2n, limbs)
        ctx = Context(p, 0)
        ev = Evaluator(ctx)
        t = torch.zeros((items, 2, limbs, p.n), dtype=torch.int64, device=ctx.device)
        for _ in range(3):
            ev.expand_uniform_(t, seed, 1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            ev.expand_uniform_(t, seed, 1)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        coeffs = items * limbs * p.n
        res["shapes"].append({"name": name, "log2n": log2n, "limbs": limbs, "items": items, "coefficients": coeffs,
                              "grid_threads": coeffs // 4, "event_us_per_launch": round(us, 2), "event_gcoef_s": round(coeffs / us / 1e3, 1)})
        print(json.dumps(res["shapes"][-1]), flush=True)
        del t
        ctx.close()
    if not args.no_load:
        res["load"] = run_load(5)
        print(json.dumps(res["load"]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(res, open(os.path.join(args.out, "run.json"), "w"), indent=1)


def isa_count():
    """VALU / SALU / all instructions of expand_uniform_kernel (straight-line: no loop, so the static count is the dynamic count per lane)"""
    d = tempfile.mkdtemp()
    out = os.path.join(d, "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(ROOT, "deeppowers_amd", "csrc", "k_expand.hip")])
    text = open(out).read()
    body = text[text.index("_ZN5dpfhe21expand_uniform_kernel"):]
    body = body[body.index(":\n") + 2: body.index("s_endpgm") + len("s_endpgm")]
    ins = [l.split(";")[0].strip() for l in body.splitlines()]
    ins = [l for l in ins if l and not l.startswith((".", "//")) and not l.endswith(":")]
    branches = [l for l in ins if l.startswith(("s_cbranch", "s_branch"))]
    assert not branches, f"the kernel is expected straight-line, found {branches}"
    c = lambda pre: sum(1 for l in ins if l.startswith(pre))
    return {"valu": c("v_"), "salu": c("s_"), "vmem": c("global_"), "all": len(ins), "v_alignbit_b32": c("v_alignbit_b32"), "v_perm_b32": c("v_perm_b32"),
            "v_lshlrev_b32": c("v_lshlrev_b32"), "v_lshrrev_b32": c("v_lshrrev_b32"), "v_or_b32": c("v_or_b32")}


def kernel_times(prof_dir):
    """per grid size: dispatches and mean / min kernel ns of expand_uniform_kernel from rocprofv3's kernel trace"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {prof_dir}")
    by = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            if "expand_uniform_kernel" not in row.get("Kernel_Name", ""):
                continue
            grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
            ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            by.setdefault(grid, []).append(ns)
    return {g: {"dispatches": len(v), "mean_ns": sum(v) / len(v), "min_ns": min(v)} for g, v in by.items()}


def report(args):
    run_res = json.load(open(args.run))
    isa = isa_count()
    prof = kernel_times(args.prof) if args.prof else {}
    valu_rate = CUS * SIMDS * CLOCK_GHZ * 1e9 / 2                 # wave64 VALU instructions per second, chip-wide
    lines = ["seeded uniform polynomials: dpfhe_expand_uniform (csrc/k_expand.hip expand_uniform_kernel) on one MI355X",
             f"ISA of expand_uniform_kernel per lane (one ChaCha20 block = 4 coefficients), straight-line: {isa['valu']} VALU, {isa['salu']} SALU, "
             f"{isa['vmem']} stores, {isa['all']} in all",
             f"  rotations: {isa['v_alignbit_b32']} v_alignbit_b32 + {isa['v_perm_b32']} v_perm_b32 (20 rounds x 16 = 320); shifts left {isa['v_lshlrev_b32']}, "
             f"right {isa['v_lshrrev_b32']}, v_or_b32 {isa['v_or_b32']} (no shift-shift-or rotations)",
             f"VALU bound: {CUS} CUs x {SIMDS} SIMDs x 1 wave64 instruction / 2 cycles x {CLOCK_GHZ} GHz = {valu_rate / 1e12:.3f} T wave-instr/s"
             f" -> {valu_rate / isa['valu'] * 256 / 1e9:.0f} G coefficients/s at {isa['valu'] / 4:.0f} VALU instructions (x 64 lanes) per coefficient", ""]
    lines.append(f"{'shape':<12} {'items':>6} {'coefficients':>13} {'kernel us (rocprofv3 mean / min)':>34} {'G coef/s':>9} {'GB/s written':>13} "
                 f"{'share of VALU bound':>20} {'event us':>9}")
    for s in run_res["shapes"]:
        k = prof.get(s["grid_threads"])
        bound_us = s["coefficients"] / (valu_rate / isa["valu"] * 256) * 1e6
        if k:
            us = k["mean_ns"] / 1e3
            lines.append(f"{s['name']:<12} {s['items']:>6} {s['coefficients']:>13} {us:>20.1f} / {k['min_ns'] / 1e3:>10.1f} ({k['dispatches']:>3})"
                         f" {s['coefficients'] / us / 1e3:>9.1f} {s['coefficients'] * 8 / us / 1e3:>13.0f} {bound_us / us:>19.1%} {s['event_us_per_launch']:>9.1f}")
        else:
            lines.append(f"{s['name']:<12} {s['items']:>6} {s['coefficients']:>13} {'(no trace)':>34} {s['event_gcoef_s']:>9.1f} "
                         f"{s['coefficients'] * 8 / s['event_us_per_launch'] / 1e3:>13.0f} {bound_us / s['event_us_per_launch']:>19.1%} {s['event_us_per_launch']:>9.1f}")
    if "load" in run_res:
        ld = run_res["load"]
        lines += ["", f"PolyBuffer::load against load_seeded, {ld['ciphertexts']} two-component ciphertexts at N = 4096 / L = 4 held in memory "
                      f"(host parse + canonical check + upload (+ expansion); best of {ld['reps']}, host clock around a device synchronise):",
                  f"  load        {ld['v1_bytes'] / 2**20:8.1f} MiB stream  {ld['load_ms']:8.1f} ms",
                  f"  load_seeded {ld['seeded_bytes'] / 2**20:8.1f} MiB stream  {ld['load_seeded_ms']:8.1f} ms  "
                  f"({ld['seeded_bytes'] / ld['v1_bytes']:.4f} of the bytes, {ld['load_seeded_ms'] / ld['load_ms']:.2f} of the time)"]
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--reps", type=int, default=50)
    r.add_argument("--no-load", action="store_true")
    r.add_argument("--out", required=True, help="directory for run.json")
    p = sub.add_parser("report")
    p.add_argument("--run", required=True)
    p.add_argument("--prof", default=None)
    sub.add_parser("isa")
    a = ap.parse_args()
    if a.cmd == "run":
        run(a)
    elif a.cmd == "report":
        report(a)
    else:
        print(json.dumps(isa_count()))


if __name__ == "__main__":
    main()
