"""Same-process A/B timing of a whole slot sum over blocks of 64 slots (tool, not on the product path; MEASUREMENTS.md "Hoisted slot sums"):
  ladder    one dpfhe_rotate_add_hybrid of 6 steps (elements 3^(2^e)) - what SlotSum runs today
  radix4    three dpfhe_rotate_sum_hoisted stages of 3 rotations (elements 3^(w k), k = 1 .. 3, w = 1, 4, 16)
  radix8    two stages of 7 rotations (w = 1, 8)
at N = 8192 and N = 32768 on 7 data limbs + P, 8 and 36 items (the LayerNorm example's shape and the 8-token causal attention's pair count).  Random
canonical words and keys: a timing, the routes' words differ by their switching noise and are held to the oracle by the tests.  Every route is warmed up;
then they alternate, WINDOWS windows each, a window being enough back-to-back sums between two device events to last at least WINDOW_SECONDS.  Per route the
median window, the fastest and the slowest, in milliseconds per sum; each hoisted route's ratio to the ladder; the spreads are the noise a difference has to
exceed.  One JSON line per shape, also appended to profiles/r24_slot_sum_radix.txt.
`stage`: instead, 20 radix-8 first stages per shape and nothing else - the run to put under a kernel trace for hoisted_qp_sum_kernel's own time; the row
states the rows the kernel requests and the rows it cannot avoid, per launch.
usage: python tools/slot_sum_radix_bench.py [windows = 10] [window_seconds = 0.5] [quick | stage]      (quick: N = 4096, Ld = 2, a rehearsal)"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.evaluator import Context  # noqa: E402
from deeppowers_amd.params import FheParams, ntt_primes  # noqa: E402

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
WINDOW_SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
MODE = sys.argv[3] if len(sys.argv) > 3 else ""
BLOCK = 64
OUT = os.path.join(ROOT, "profiles", "r24_slot_sum_radix.txt")


def words(gen, moduli, lead, n, dev):
    q = torch.tensor(moduli, dtype=torch.int64, device=dev).view(-1, 1)
    return torch.randint(0, 2 ** 62, tuple(lead) + (len(moduli), n), generator=gen, dtype=torch.int64, device=dev) % q


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stages(radix, n):
    """[(elements of stage s)]: radix rho while log2(rho) bits of log2(BLOCK) remain, then the remainder; weight w_s = the product of the radices before it"""
    out, w, left = [], 1, BLOCK
    while left > 1:
        rho = min(radix, left)
        out.append([pow(3, w * k, 2 * n) for k in range(1, rho)])
        w, left = w * rho, left // rho
    return out


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def shape(ext_params, T):
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    g = torch.Generator(device=dev).manual_seed(11)
    new = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    x = words(g, ext_params.moduli[:Ld], (T, 2), n, dev)
    ping, pong, in_ntt, digits, sum_qp = new(T, 2, Ld, n), new(T, 2, Ld, n), new(T, 2, Ld, n), new(T, Ld, L, n), new(T, 2, L, n)
    work, acc = new(T, 2, L, n), new(T, 2, Ld, n)

    def hoisted(radix):
        plan = [((C.c_uint32 * len(e))(*e), len(e), words(g, ext_params.moduli, (len(e), Ld, 2), n, dev)) for e in stages(radix, n)]

        def run():
            cur = x
            for i, (elts, R, keys) in enumerate(plan):
                dst = pong if (len(plan) - 1 - i) & 1 else ping
                _cabi.check(lib.dpfhe_rotate_sum_hoisted(ext.handle, dst.data_ptr(), cur.data_ptr(), T, elts, keys.data_ptr(), R, in_ntt.data_ptr(), digits.data_ptr(),
                                                         sum_qp.data_ptr(), None), "dpfhe_rotate_sum_hoisted")
                cur = dst
        return run, plan

    if MODE == "stage":
        run, plan = hoisted(8)
        elts, R, keys = plan[0]
        one = lambda: _cabi.check(lib.dpfhe_rotate_sum_hoisted(ext.handle, ping.data_ptr(), x.data_ptr(), T, elts, keys.data_ptr(), R, in_ntt.data_ptr(), digits.data_ptr(),
                                                               sum_qp.data_ptr(), None), "dpfhe_rotate_sum_hoisted")
        ms = timed(one, 20)
        row_bytes = n * 8
        emit({"mode": "stage", "log2_n": ext_params.log2_n, "data_limbs": Ld, "items": T, "rotations": R, "entry_ms": round(ms, 4),
              "kernel_rows_requested": T * (R * (Ld + 1) * Ld + R * Ld + 2 * L) + -(-T // 4) * R * 2 * Ld * L,
              "kernel_rows_algorithmic": T * (Ld * L + Ld + 2 * L) + R * 2 * Ld * L, "row_bytes": row_bytes})
        ext.close()
        return
    steps = BLOCK.bit_length() - 1
    l_elts = (C.c_uint32 * steps)(*[pow(3, 1 << e, 2 * n) for e in range(steps)])
    l_keys = words(g, ext_params.moduli, (steps, Ld, 2), n, dev)
    ladder = lambda: _cabi.check(lib.dpfhe_rotate_add_hybrid(ext.handle, ping.data_ptr(), x.data_ptr(), l_elts, l_keys.data_ptr(), work.data_ptr(), acc.data_ptr(), steps, T,
                                                             None), "dpfhe_rotate_add_hybrid")
    routes = {"ladder": ladder, "radix4": hoisted(4)[0], "radix8": hoisted(8)[0]}
    for f in routes.values():
        f()
        f()
    torch.cuda.synchronize()
    reps = {name: max(1, int(WINDOW_SECONDS * 1e3 / timed(f, 3)) + 1) for name, f in routes.items()}
    ms = {name: [] for name in routes}
    for _ in range(WINDOWS):
        for name, f in routes.items():
            ms[name].append(timed(f, reps[name]))
    row = {"block": BLOCK, "log2_n": ext_params.log2_n, "data_limbs": Ld, "items": T, "windows": WINDOWS, "window_seconds": WINDOW_SECONDS}
    for name, v in ms.items():
        v.sort()
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "sums_per_window": reps[name],
                             "spread": round((v[-1] - v[0]) / v[len(v) // 2], 4)}
    for name in ("radix4", "radix8"):
        row[name + "_over_ladder"] = round(row[name + "_ms"]["median"] / row["ladder_ms"]["median"], 4)
    emit(row)
    ext.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        shape(ntt_primes(12, 3), 5)
    else:
        for params in (FheParams.n8192(8), FheParams.n32768(8)):
            for T in (8, 36):
                shape(params, T)
