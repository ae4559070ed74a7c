"""Two builds of libdpfhe_hip.so against each other (tool; profiles/r20_last_pass_refactor.txt): another commit's library and this tree's are loaded into ONE
process and the same entry runs on the same buffers, alternating round by round.  Two sets of entries: "streaming" (the default) - the streaming kernels of
key switching, dpfhe_rescale, dpfhe_rescale_bsgs, dpfhe_lincomb_rescale, dpfhe_relinearize_lincomb_rescale_hybrid, on fold and generic primes; "arenas"
(profiles/r22_scratch_leases.txt) - the composed dpfhe_ct_mul and dpfhe_relinearize at N = 16384, L = 3, batch 1 and 8, one stream in steady state, which
lease their stream's scratch arena.  Per shape: median / min / max ms per call of each library by events, and us of host time per call (the enqueue cost: the
wall time of the calls alone), whether this tree's median lies inside the other's own min-max range (the noise, measured in the same run), and whether both
libraries wrote the same words.
usage: python tools/lib_ab_bench.py <the other build's libdpfhe_hip.so> [rounds = 9] [reps = 20] [streaming | arenas]"""
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.params import ntt_primes  # noqa: E402

ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
SET = sys.argv[4] if len(sys.argv) > 4 else "streaming"


def load(path):
    lib = C.CDLL(path)
    for name, (argtypes, restype) in _cabi.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


LIBS = {"parent": load(os.path.abspath(sys.argv[1])), "new": load(_cabi.LIB_PATH)}
DEV = torch.device("cuda", 0)


def ctx_of(lib, params):
    L = params.n_limbs
    h = C.c_void_p()
    rc = lib.dpfhe_ctx_create(C.byref(h), params.log2_n, L, (C.c_uint64 * L)(*params.moduli), (C.c_uint64 * L)(*params.psi), 0)
    assert rc == 0, lib.dpfhe_last_error()
    return h


def words(gen, moduli, lead, n):
    q = torch.tensor(moduli, dtype=torch.int64, device=DEV).view(-1, 1)
    return torch.randint(0, 2 ** 62, tuple(lead) + (len(moduli), n), generator=gen, dtype=torch.int64, device=DEV) % q


def ok(lib, rc):
    assert rc == 0, lib.dpfhe_last_error()


def alternate(what, shape, calls, outs):
    """calls: name -> callable enqueueing one call; outs: name -> output tensor"""
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    ms, host = {name: [] for name in calls}, {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(REPS):
                f()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / REPS)
            host[name].append((t1 - t0) * 1e6 / REPS)
    row = {"entry": what, **shape, "rounds": ROUNDS, "reps": REPS, "same_words": bool(torch.equal(outs["parent"], outs["new"]))}
    for name, v in ms.items():
        v.sort()
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 5), "min": round(v[0], 5), "max": round(v[-1], 5)}
    p, nw = ms["parent"], ms["new"]
    row["new_over_parent"] = round(nw[len(nw) // 2] / p[len(p) // 2], 4)
    row["new_median_inside_parent_range"] = bool(p[0] <= nw[len(nw) // 2] <= p[-1])
    row["new_median_not_above_parent_max"] = bool(nw[len(nw) // 2] <= p[-1])
    for name, v in host.items():
        v.sort()
        row[name + "_host_us"] = {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}
    p, nw = host["parent"], host["new"]
    row["new_minus_parent_host_us"] = round(nw[len(nw) // 2] - p[len(p) // 2], 2)
    row["new_host_median_inside_parent_range"] = bool(p[0] <= nw[len(nw) // 2] <= p[-1])
    print(json.dumps(row), flush=True)


def rescale(params, polys, tag):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = words(g, params.moduli, (polys,), params.n)
    calls, outs, keep = {}, {}, []
    for name, lib in LIBS.items():
        h = ctx_of(lib, params)
        out = torch.zeros((polys, params.n_limbs - 1, params.n), dtype=torch.int64, device=DEV)
        calls[name] = lambda lib=lib, h=h, out=out: ok(lib, lib.dpfhe_rescale(h, out.data_ptr(), x.data_ptr(), polys, None))
        outs[name] = out
        keep.append(h)
    alternate("dpfhe_rescale", {"arith": tag, "log2_n": params.log2_n, "limbs": params.n_limbs, "polys": polys, "fold": LIBS["new"].dpfhe_ctx_uses_fold(keep[-1])}, calls, outs)


def rescale_bsgs(ext, batch, n_add, tag):
    L, Ld, n = ext.n_limbs, ext.n_limbs - 1, ext.n
    g = torch.Generator(device=DEV).manual_seed(4)
    x = words(g, ext.moduli, (batch, 2), n)
    add = words(g, ext.moduli[:Ld], (n_add, batch, 2), n)
    calls, outs, keep = {}, {}, []
    for name, lib in LIBS.items():
        h = ctx_of(lib, ext)
        out = torch.zeros((batch, 2, Ld, n), dtype=torch.int64, device=DEV)
        calls[name] = lambda lib=lib, h=h, out=out: ok(lib, lib.dpfhe_rescale_bsgs(h, out.data_ptr(), x.data_ptr(), add.data_ptr(), n_add, batch, None))
        outs[name] = out
        keep.append(h)
    alternate("dpfhe_rescale_bsgs", {"arith": tag, "log2_n": ext.log2_n, "limbs": L, "batch": batch, "n_add": n_add, "fold": LIBS["new"].dpfhe_ctx_uses_fold(keep[-1])}, calls, outs)


def lincomb(params, K, T, tag):
    L, n = params.n_limbs, params.n
    g = torch.Generator(device=DEV).manual_seed(9)
    x = words(g, params.moduli, (K, T, 2), n)
    q = torch.tensor(params.moduli, dtype=torch.int64, device=DEV)
    w = torch.randint(0, 2 ** 62, (K + 1, L), generator=g, dtype=torch.int64, device=DEV) % q
    calls, outs, keep = {}, {}, []
    for name, lib in LIBS.items():
        h = ctx_of(lib, params)
        out = torch.zeros((T, 2, L - 1, n), dtype=torch.int64, device=DEV)
        calls[name] = lambda lib=lib, h=h, out=out: ok(lib, lib.dpfhe_lincomb_rescale(h, out.data_ptr(), x.data_ptr(), w.data_ptr(), K, T, None))
        outs[name] = out
        keep.append(h)
    alternate("dpfhe_lincomb_rescale", {"arith": tag, "log2_n": params.log2_n, "limbs": L, "terms": K, "tokens": T, "fold": LIBS["new"].dpfhe_ctx_uses_fold(keep[-1])}, calls, outs)


def relin_lincomb(ext, K, batch, tag):
    L, Ld, n = ext.n_limbs, ext.n_limbs - 1, ext.n
    g = torch.Generator(device=DEV).manual_seed(7)
    in3 = words(g, ext.moduli[:Ld], (batch, 3), n)
    key = words(g, ext.moduli, (Ld, 2), n)
    terms = [words(g, ext.moduli[:Ld], (batch, 2), n) for _ in range(K)]
    q = torch.tensor(ext.moduli[:Ld], dtype=torch.int64, device=DEV)
    w = torch.randint(0, 2 ** 62, (K + 2, Ld), generator=g, dtype=torch.int64, device=DEV) % q
    ptrs = (C.c_void_p * max(K, 1))(*[t.data_ptr() for t in terms])
    limbs = (C.c_uint32 * max(K, 1))(*[Ld] * K)
    calls, outs, keep = {}, {}, []
    for name, lib in LIBS.items():
        h = ctx_of(lib, ext)
        work = torch.zeros((batch, 2, L, n), dtype=torch.int64, device=DEV)
        out = torch.zeros((batch, 2, Ld - 1, n), dtype=torch.int64, device=DEV)
        calls[name] = lambda lib=lib, h=h, out=out, work=work: ok(lib, lib.dpfhe_relinearize_lincomb_rescale_hybrid(
            h, out.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), ptrs, limbs, K, w.data_ptr(), batch, None))
        outs[name] = out
        keep.append((h, work))
    alternate("dpfhe_relinearize_lincomb_rescale_hybrid", {"arith": tag, "log2_n": ext.log2_n, "data_limbs": Ld, "terms": K, "batch": batch,
                                                           "fold": LIBS["new"].dpfhe_ctx_uses_fold(keep[-1][0])}, calls, outs)


def composed(params, batch, relin):
    """dpfhe_ct_mul / dpfhe_relinearize above N = 8192: composed, scratch leased from the null stream's arena"""
    L, n = params.n_limbs, params.n
    g = torch.Generator(device=DEV).manual_seed(5)
    x = words(g, params.moduli, (batch, 3 if relin else 2), n)
    y = words(g, params.moduli, (L, 2) if relin else (batch, 2), n)
    calls, outs, keep = {}, {}, []
    for name, lib in LIBS.items():
        h = ctx_of(lib, params)
        out = torch.zeros((batch, 2 if relin else 3, L, n), dtype=torch.int64, device=DEV)
        if relin:
            calls[name] = lambda lib=lib, h=h, out=out: ok(lib, lib.dpfhe_relinearize(h, out.data_ptr(), x.data_ptr(), y.data_ptr(), batch, None))
        else:
            calls[name] = lambda lib=lib, h=h, out=out: ok(lib, lib.dpfhe_ct_mul(h, out.data_ptr(), x.data_ptr(), y.data_ptr(), batch, 0, None))
        outs[name] = out
        keep.append(h)
    for f in calls.values():   # the arenas exist from here on
        f()
    torch.cuda.synchronize()
    alternate("dpfhe_relinearize" if relin else "dpfhe_ct_mul", {"log2_n": params.log2_n, "limbs": L, "batch": batch, "scratch_bytes": LIBS["new"].dpfhe_ctx_scratch_bytes(keep[-1])},
              calls, outs)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if SET == "arenas":
        for batch in (1, 8):
            for relin in (False, True):
                composed(ntt_primes(14, 3), batch, relin)
        sys.exit(0)
    fold13, gen13 = ntt_primes(13, 6), ntt_primes(13, 6, 58)
    for params, tag in ((fold13, "fold"), (gen13, "generic")):
        rescale(params, 128, tag)
        rescale_bsgs(params, 16, 8, tag)
        for K in (4, 15):
            lincomb(ntt_primes(13, 4, 60 if tag == "fold" else 58), K, 8, tag)
        for K in (1, 15):
            relin_lincomb(params, K, 64, tag)
    for K in (4, 15):
        lincomb(ntt_primes(15, 4), K, 8, "fold")
