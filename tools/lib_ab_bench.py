"""Two builds of libdpfhe_hip.so against each other (tool; profiles/r20_last_pass_refactor.txt): another commit's library and this tree's are loaded into ONE
process and the same entry runs on the same buffers, alternating round by round, for the streaming kernels of key switching - dpfhe_rescale, dpfhe_rescale_bsgs,
dpfhe_lincomb_rescale, dpfhe_relinearize_lincomb_rescale_hybrid - on fold and generic primes.  Per shape: median / min / max ms per call of each library, whether
this tree's median lies inside the other's own min-max range (the noise, measured in the same run), and whether both libraries wrote the same words.
usage: python tools/lib_ab_bench.py <the other build's libdpfhe_hip.so> [rounds = 9] [reps = 20]"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.params import ntt_primes  # noqa: E402

ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20


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
    ms = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / REPS)
    row = {"entry": what, **shape, "rounds": ROUNDS, "reps": REPS, "same_words": bool(torch.equal(outs["parent"], outs["new"]))}
    for name, v in ms.items():
        v.sort()
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 5), "min": round(v[0], 5), "max": round(v[-1], 5)}
    p, nw = ms["parent"], ms["new"]
    row["new_over_parent"] = round(nw[len(nw) // 2] / p[len(p) // 2], 4)
    row["new_median_inside_parent_range"] = bool(p[0] <= nw[len(nw) // 2] <= p[-1])
    row["new_median_not_above_parent_max"] = bool(nw[len(nw) // 2] <= p[-1])
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


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
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
