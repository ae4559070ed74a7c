"""Same-process A/B timing of the encrypted attention scores against what they replace (tool; MEASUREMENTS.md "Attention scores"):
  (a) dpfhe_ct_mul_outer (coefficient domain in and out)
          against  dpfhe_ct_mul on the two pair lists, which the tool materialises with dpfhe_copy item by item - the copies are timed as a form of their own
          and reported separately, so that the multiply alone and the multiply with its copies can both be read off - the same words;
  (b) the WHOLE scores step (ApproxAttentionScores::apply): dpfhe_ct_mul_outer + dpfhe_relinearize_rescale_hybrid over all pairs + the rotate-and-add ladder
          of GPT-2's interleaved heads (block 64, stride 16: 6 steps of dpfhe_rotate_add_hybrid on the next level)
          against  dpfhe_ct_mul on the pair lists + the same two entries - the same words.  The baseline does NOT include the copies (the headline compares
          against pair lists that cost nothing); `pair_list_step_with_copies` adds them, as a caller without the entry would run it today;
  at N = 8192 and N = 32768, 7 data limbs, T = 8 and 32 queries and keys, full and causal.
After a warm-up of every shape the forms alternate, ROUNDS rounds of REPS back-to-back calls each between two events; per form the median round, the fastest
and the slowest are printed (the spread of the baseline is the noise a difference has to exceed), and both parts assert the same words first.
usage: python tools/attention_scores_bench.py [rounds = 7] [reps = 10] [all | quick]"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.evaluator import Context  # noqa: E402
from deeppowers_amd.params import FheParams, ntt_primes  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
MODE = sys.argv[3] if len(sys.argv) > 3 else "all"
TILE = 4
BLOCK, STRIDE = 64, 16          # GPT-2 small's 12 heads of 64, interleaved at stride 16: a 6-step ladder


def words(gen, moduli, lead, n, dev):
    q = torch.tensor(moduli, dtype=torch.int64, device=dev).view(-1, 1)
    return torch.randint(0, 2 ** 62, tuple(lead) + (len(moduli), n), generator=gen, dtype=torch.int64, device=dev) % q


def alternate(forms):
    """forms: name -> callable enqueueing one call.  -> name -> sorted milliseconds per call, one per round"""
    for f in forms.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(ROUNDS):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / REPS)
    return {name: sorted(v) for name, v in ms.items()}


def report(row, ms, base, new):
    for name, v in ms.items():
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    b, f = ms[base], ms[new]
    row[f"{new}_over_{base}"] = round(f[len(f) // 2] / b[len(b) // 2], 4)
    row[f"{base}_spread"] = round((b[-1] - b[0]) / b[len(b) // 2], 4)
    print(json.dumps(row), flush=True)


def shape(ext_params, T, causal):
    """ext_params: the extended context (Ld data limbs + P)"""
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    data_params = ext_params.drop_last_limb()
    data = Context(data_params, 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    g = torch.Generator(device=dev).manual_seed(17)
    a = words(g, data_params.moduli, (T, 2), n, dev)
    b = words(g, data_params.moduli, (T, 2), n, dev)
    key = words(g, ext_params.moduli, (Ld, 2), n, dev)
    idx = [(i, j) for i in range(T) for j in range(T) if not causal or j <= i]
    pairs = len(idx)
    z = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    out_new, out_old, la, lb = z(pairs, 3, Ld, n), z(pairs, 3, Ld, n), z(pairs, 2, Ld, n), z(pairs, 2, Ld, n)
    p = lambda t: t.data_ptr()
    flags = _cabi.OUTER_CAUSAL if causal else 0
    item = 2 * Ld * n
    base = {"log2_n": ext_params.log2_n, "data_limbs": Ld, "T": T, "causal": causal, "pairs": pairs, "rounds": ROUNDS, "reps": REPS}

    def outer():
        _cabi.check(lib.dpfhe_ct_mul_outer(data.handle, p(out_new), p(a), p(b), T, T, flags, None), "dpfhe_ct_mul_outer")

    def copies():
        for k, (i, j) in enumerate(idx):
            _cabi.check(lib.dpfhe_copy(data.handle, p(la[k]), p(a[i]), item, None), "dpfhe_copy")
            _cabi.check(lib.dpfhe_copy(data.handle, p(lb[k]), p(b[j]), item, None), "dpfhe_copy")

    def ct_mul():
        _cabi.check(lib.dpfhe_ct_mul(data.handle, p(out_old), p(la), p(lb), pairs, 0, None), "dpfhe_ct_mul")

    # ---- (a) the tensor products
    ms = alternate({"ct_mul_pair_lists": ct_mul, "copies": copies, "outer": outer})
    same = bool(torch.equal(out_new, out_old))
    tiles = -(-T // TILE)
    report(dict(base, part="a", entry="dpfhe_ct_mul_outer", same_words=same,
                rows_per_limb={"outer_read": 2 * T + 2 * T * tiles, "pair_lists_read": 4 * pairs, "written": 3 * pairs, "copies_read_and_written": 4 * pairs}),
           ms, "ct_mul_pair_lists", "outer")
    assert same, "dpfhe_ct_mul_outer and dpfhe_ct_mul on the pair lists gave different words"

    # ---- (b) the whole scores step: product, key switch + rescale, and the ladder on the next level
    nxt_params = data_params.drop_last_limb()
    ext2_params = FheParams(ext_params.log2_n, tuple(nxt_params.moduli) + (ext_params.moduli[-1],), tuple(nxt_params.psi) + (ext_params.psi[-1],))
    ext2 = Context(ext2_params, 0)
    L2, Ld2 = ext2_params.n_limbs, ext2_params.n_limbs - 1
    elts, e = [], pow(3, STRIDE, 2 * n)
    while len(elts) < BLOCK.bit_length() - 1:
        elts.append(e)
        e = e * e % (2 * n)
    c_elts = (C.c_uint32 * len(elts))(*elts)
    lkeys = words(g, ext2_params.moduli, (len(elts), Ld2, 2), n, dev)
    work = z(pairs, 2, L, n)
    lwork, lacc = z(pairs, 2, L2, n), z(pairs, 2, Ld2, n)
    step_new, step_old, sc_new, sc_old = z(pairs, 2, Ld - 1, n), z(pairs, 2, Ld - 1, n), z(pairs, 2, Ld2, n), z(pairs, 2, Ld2, n)

    def tail(prod, step, scores):
        _cabi.check(lib.dpfhe_relinearize_rescale_hybrid(ext.handle, p(step), p(prod), p(key), p(work), pairs, None), "dpfhe_relinearize_rescale_hybrid")
        _cabi.check(lib.dpfhe_rotate_add_hybrid(ext2.handle, p(scores), p(step), c_elts, p(lkeys), p(lwork), p(lacc), len(elts), pairs, None), "dpfhe_rotate_add_hybrid")

    def scores_step():
        outer()
        tail(out_new, step_new, sc_new)

    def pair_list_step():
        ct_mul()
        tail(out_old, step_old, sc_old)

    def pair_list_step_with_copies():
        copies()
        pair_list_step()
    ms = alternate({"pair_list_step": pair_list_step, "pair_list_step_with_copies": pair_list_step_with_copies, "scores_step": scores_step})
    same = bool(torch.equal(sc_new, sc_old))
    row = dict(base, part="b", entry="ApproxAttentionScores::apply", same_words=same, key_switches={"product": pairs, "ladder": pairs * len(elts)})
    v, w = ms["scores_step"], ms["pair_list_step_with_copies"]
    row["scores_step_over_pair_list_step_with_copies"] = round(v[len(v) // 2] / w[len(w) // 2], 4)
    report(row, ms, "pair_list_step", "scores_step")
    assert same, "the two scores steps gave different words"
    del lkeys, lwork, lacc, sc_new, sc_old
    ext2.close()
    del a, b, key, out_new, out_old, la, lb, work, step_new, step_old
    torch.cuda.empty_cache()
    for c in (data, ext):
        c.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        shape(ntt_primes(12, 4), 5, True)
    else:
        for params in (FheParams.n8192(8), FheParams.n32768(8)):
            for T in (8, 32):
                for causal in (False, True):
                    shape(params, T, causal)
