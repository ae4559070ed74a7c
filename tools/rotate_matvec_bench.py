"""Same-process A/B timing of the first two stages of a packed layer (tool, not on the product path; MEASUREMENTS.md "Baby steps fused with their diagonal
products"):
  two     dpfhe_rotate_hoisted_qp into a (1 + R) T block buffer, then dpfhe_matvec_plain_multi over it - what PackedLinear::apply runs by default
  fused   dpfhe_rotate_matvec_hoisted_qp - the same words, no block buffer
on 7 data limbs + P at N = 8192 and N = 32768, 1 and 8 tokens, at PackedLinear's split of GPT-2 small's layers: 768 x 768 and 768 -> 3072 both pad to 1024
diagonals = 64 baby x 16 giant steps in one output ciphertext, so both are R = 63 rotations and 16 rows of W (only the diagonals' values differ).  Random
canonical words: a timing; the words are held to the oracle by tests/test_gpu_rotate_matvec.py.  Both routes are warmed up; then they alternate, WINDOWS
windows each, a window being enough back-to-back calls between two device events to last at least WINDOW_SECONDS.  Per route the median window, the fastest
and the slowest in milliseconds per call, and fused / two; the spreads are the noise a difference has to exceed.  One JSON line per shape, also appended to
profiles/r25_rotate_matvec.txt.
usage: python tools/rotate_matvec_bench.py [windows = 10] [window_seconds = 0.5] [quick]      (quick: N = 4096, Ld = 2, a rehearsal)"""
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
OUT = os.path.join(ROOT, "profiles", "r25_rotate_matvec.txt")
ROW_TILE = 6   # csrc/workmap.h kRotMatvecRows


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


def shape(ext_params, T, R, rows):
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    g = torch.Generator(device=dev).manual_seed(12)
    new = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    x = words(g, ext_params.moduli[:Ld], (T, 2), n, dev)
    keys = words(g, ext_params.moduli, (R, Ld, 2), n, dev)
    W = words(g, ext_params.moduli, (rows, R + 1), n, dev)
    elts = (C.c_uint32 * R)(*[pow(3, k, 2 * n) for k in range(1, R + 1)])
    blocks, y, in_ntt, digits = new(R + 1, T, 2, L, n), new(rows, T, 2, L, n), new(T, 2, Ld, n), new(T, Ld, L, n)

    def two():
        _cabi.check(lib.dpfhe_rotate_hoisted_qp(ext.handle, blocks.data_ptr(), x.data_ptr(), T, elts, keys.data_ptr(), in_ntt.data_ptr(), digits.data_ptr(), R, None),
                    "dpfhe_rotate_hoisted_qp")
        _cabi.check(lib.dpfhe_matvec_plain_multi(ext.handle, y.data_ptr(), W.data_ptr(), blocks.data_ptr(), rows, R + 1, T, None), "dpfhe_matvec_plain_multi")

    def fused():
        _cabi.check(lib.dpfhe_rotate_matvec_hoisted_qp(ext.handle, y.data_ptr(), W.data_ptr(), x.data_ptr(), T, elts, keys.data_ptr(), R, rows, in_ntt.data_ptr(),
                                                       digits.data_ptr(), None), "dpfhe_rotate_matvec_hoisted_qp")

    routes = {"two": two, "fused": fused}
    outs = {}
    for name, f in routes.items():
        f()
        f()
        torch.cuda.synchronize()
        outs[name] = y.clone()
    reps = {name: max(1, int(WINDOW_SECONDS * 1e3 / timed(f, 3)) + 1) for name, f in routes.items()}
    ms = {name: [] for name in routes}
    for _ in range(WINDOWS):
        for name, f in routes.items():
            ms[name].append(timed(f, reps[name]))
    tiles = -(-rows // ROW_TILE)
    row = {"log2_n": ext_params.log2_n, "data_limbs": Ld, "tokens": T, "rotations": R, "rows": rows, "windows": WINDOWS, "window_seconds": WINDOW_SECONDS,
           "same_words": bool(torch.equal(outs["two"], outs["fused"])), "row_bytes": n * 8,
           # rows of N words each side cannot avoid (HBM, every operand once) beyond the shared lift (T (2 Ld + Ld L) transforms' traffic on both sides)
           "rows_algorithmic": {"two": R * 2 * Ld * L + T * (Ld * L + 2 * Ld) + 2 * (R + 1) * T * 2 * L + rows * (R + 1) * L + rows * T * 2 * L,
                                "fused": R * 2 * Ld * L + T * (Ld * L + 2 * Ld) + rows * (R + 1) * L + rows * T * 2 * L},
           "key_products_formed": {"two": 1, "fused": tiles}}     # times each rotated key product is computed: once per tile of ROW_TILE rows when fused
    for name, v in ms.items():
        v.sort()
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "calls_per_window": reps[name],
                             "spread": round((v[-1] - v[0]) / v[len(v) // 2], 4)}
    row["fused_over_two"] = round(row["fused_ms"]["median"] / row["two_ms"]["median"], 4)
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")
    ext.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        shape(ntt_primes(12, 3), 3, 9, 7)
    else:
        for params in (FheParams.n8192(8), FheParams.n32768(8)):
            for T in (1, 8):
                shape(params, T, 63, 16)
