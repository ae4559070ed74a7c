"""-m gpu: the fused baby steps x diagonals of the packed layers (include/dpfhe.h dpfhe_rotate_matvec_hoisted_qp; csrc/rotate_matvec.h, workmap.h RotMatvecMap),
word for word against the oracle - Oracle.rotate_hoisted_qp's blocks, then the oracle's matvec on the extended context, as tests/test_gpu_bsgs_qp.py and
tests/test_gpu_footprint.py compose them - and against the device composition of the two entries it replaces.  Inputs are Rig.words (stripes in item 0,
q - 1 in every word of item 1, of key 1 and of row 1 of W).  Also: the footprint case, the rejections and the packed layer with the option on."""
import json
import subprocess

import numpy as np
import pytest

import test_gpu_footprint as fp
from class_edges import Rig, adversarial_key, edge_chain
from deeppowers_amd.evaluator import Ciphertext, Context, Plaintext, to_host
from deeppowers_amd.params import FheParams

pytestmark = pytest.mark.gpu

ROW_TILE = 6   # csrc/workmap.h kRotMatvecRows
# (chain, log2 N, L, rotations, rows, items): L = 3 / 9 are 3 / 9 key-product terms on a data limb (one side and the other of the fold after the eighth), L = 8
# and 10 the rungs beside; 9 rotations + block 0 are ten weights per row (past the rows' fold); 7 rows = a tile and a remainder tile; 3 items
SHAPES = [("fold", 8, 3, 1, 1, 1), ("fold", 8, 9, 9, 7, 3), ("fold", 8, 3, 9, 7, 1), ("fold", 8, 9, 1, 1, 3), ("fold", 8, 10, 9, 1, 1), ("fold", 13, 3, 9, 1, 3),
          ("fold", 13, 9, 1, 7, 1), ("fold", 13, 8, 9, 7, 1), ("fold", 13, 9, 9, 7, 3), ("fold", 15, 3, 1, 7, 3), ("mixed16", 12, 16, 1, 7, 3)]


@pytest.fixture
def rig():
    made = []

    def make(kind, log2n, L):
        made.append(Rig(edge_chain(kind, log2n, None if kind == "mixed16" else L)))
        return made[-1]
    yield make
    for r in made:
        r.close()


def inputs(r, R, rows, T, seed):
    """(R elements, their keys, W [rows][1 + R][L][N], T items)"""
    n = r.n
    e = [3, pow(3, -1, 2 * n), 5, n + 1, 2 * n - 1, 2 * n - 3, pow(3, 77, 2 * n), 1, pow(3, n // 4, 2 * n)] + [pow(5, i, 2 * n) for i in range(2, R)]
    return (e[:R], r.words(r.orc, (max(R, 2), r.L - 1, 2), seed)[:R], r.words(r.orc, (max(rows, 2), R + 1), seed + 1)[:rows],
            r.words(fp.data_oracle(r), (max(T, 2), 2), seed + 2)[:T])


def reference(r, cts, elts, keys, W):
    rows, cols = W.shape[:2]
    per_item = []
    for t in range(cts.shape[0]):
        blocks = r.orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0)                              # [1 + R][2][L][N]
        per_item.append(np.asarray(r.orc.matvec_plain(W.ravel(), np.ascontiguousarray(blocks).ravel(), rows, cols, threads=0)).reshape(rows, 2, r.L, r.n))
    return np.stack(per_item, axis=1)                                                                # [rows][T][2][L][N]


def fused(r, cts, elts, keys, W):
    return to_host(r.ev.rotate_matvec_hoisted_qp(r.dev(W), Ciphertext(r.dev(cts)), elts, r.dev(keys)))


@pytest.mark.parametrize("kind,log2n,L,R,rows,T", SHAPES, ids=[f"{k}_n{1 << ln}_L{L}_r{R}_rows{rows}_x{T}" for k, ln, L, R, rows, T in SHAPES])
def test_equals_the_oracle_and_the_two_entries(rig, kind, log2n, L, R, rows, T):
    r = rig(kind, log2n, L)
    elts, keys, W, cts = inputs(r, R, rows, T, 910)
    got, want = fused(r, cts, elts, keys, W), reference(r, cts, elts, keys, W)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4], got.shape)
    blocks = r.ev.rotate_hoisted_qp(Ciphertext(r.dev(cts)), elts, r.dev(keys))
    assert np.array_equal(got, to_host(r.ev.matvec_plain_multi(Plaintext(r.dev(W), True), blocks, T)))


@pytest.mark.parametrize("log2n", [8, 13])
def test_adversarial_keys_and_weights_fill_every_lazy_column(rig, log2n):
    """fold, Ld = 7 (eight key-product terms with P c0), the 64 rotations and the 6 rows one workgroup takes: rotation g's key is perm_g of the adversarial key
    of the item's digits, so every key product added lazily is q - 1 (tests/test_gpu_digit_ladder.py holds adversarial_key to its claim), and every word
    of W is q - 1"""
    r = rig("fold", log2n, 8)
    (elts, _, _, cts), orc = inputs(r, 64, 1, 1, 930), r.orc
    key = adversarial_key(orc, cts[0, 1], 931)[0]
    keys = np.stack([orc.ntt_fwd(orc.apply_galois(orc.ntt_inv(key, threads=0), g), threads=0) for g in elts])
    W = np.broadcast_to(r.qcol - np.uint64(1), (ROW_TILE, 65, r.L, r.n)).copy()
    assert np.array_equal(fused(r, cts, elts, keys, W), reference(r, cts, elts, keys, W))


def arena_cases(r, shapes=((3, 7, 2),)):
    """every buffer carved out of one arena at 16-byte alignment between guard bands, scratch at exactly the header's sizes"""
    lib, h, L, n, Ld = r.ctx._lib, r.ctx.handle, r.L, r.n, r.L - 1
    for R, rows, T in shapes:
        elts, keys, W, cts = inputs(r, R, rows, T, 940)
        c = fp.Case(r)
        c.inp("in2", cts, 2 * Ld * n)
        c.inp("keys", keys, Ld * 2 * L * n)
        c.inp("W", W, L * n)
        c.scratch("in_ntt", T * 2 * Ld * n, 2 * Ld * n)
        c.scratch("digits", T * Ld * L * n, Ld * L * n)
        c.out("y", rows * T * 2 * L * n, 2 * L * n, reference(r, cts, elts, keys, W))
        c.run(f"dpfhe_rotate_matvec_hoisted_qp {R} rotations x {rows} rows x{T}",
              lambda at: lib.dpfhe_rotate_matvec_hoisted_qp(h, at("y"), at("W"), at("in2"), T, fp.u32(elts), at("keys"), R, rows, at("in_ntt"), at("digits"), at.stream))


def test_footprint(rig):
    arena_cases(rig("fold", 12, 4))


def test_device_entry_rejects_bad_arguments(rig):
    import torch
    r = rig("fold", 8, 3)
    lib, h, L, Ld, n = r.ctx._lib, r.ctx.handle, r.L, r.L - 1, r.n
    fill = lambda *s: torch.full(s, 7, dtype=torch.int64, device=r.ctx.device)
    t = {"y": fill(2, 1, 2, L, n), "W": fill(2, 66, L, n), "in": fill(1, 2, Ld, n), "keys": fill(65, Ld, 2, L, n), "in_ntt": fill(1, 2, Ld, n), "digits": fill(1, Ld, L, n)}
    a = dict({k: v.data_ptr() for k, v in t.items()}, elts=fp.u32([3] * 65), batch=2, rows=2)

    def call(handle=h, items=1, **kw):
        b = dict(a, **kw)
        return lib.dpfhe_rotate_matvec_hoisted_qp(handle, b["y"], b["W"], b["in"], items, b["elts"], b["keys"], b["batch"], b["rows"], b["in_ntt"], b["digits"], None)
    assert call(batch=0) == call(batch=65) == call(rows=0) == call(rows=65537) == 2000                         # the ranges
    assert call(elts=fp.u32([3, 4])) == call(elts=fp.u32([2 * n + 1, 3])) == 2000                             # even, >= 2N
    for name in t:
        assert call(**{name: a[name] + 8}) == 2000 and call(**{name: None}) == 2000                           # misaligned, null
    assert call(y=a["in"]) == call(y=a["W"]) == call(digits=a["keys"]) == call(in_ntt=a["in"]) == call(in_ntt=a["digits"]) == 2000      # overlaps
    assert call(items=1 << 40) == 2000                                                                        # a grid too large for one launch
    lone = Context(FheParams(8, tuple(r.p.moduli[:1]), tuple(r.p.psi[:1])), 0)                               # no special prime
    code = call(handle=lone.handle)
    lone.close()
    torch.cuda.synchronize()
    assert code == 2002 and call(items=0) == 0 and bool((t["y"] == 7).all())                                  # every refusal left the output untouched


def test_packed_layer_with_the_option_on_gives_the_same_words():
    """examples/encrypted_gpt2_linear with its last argument `fused`: a second PackedLinear with fuse_baby_steps on, applied to the same 2 tokens at N = 8192,
    and its output ciphertexts compared word for word with the first layer's"""
    from test_gpu_cpp_api import build_example
    out = subprocess.run([build_example("encrypted_gpt2_linear"), "64x64", "1", "json", "2", "13", "1", "fused"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["correct"] is True and rec["fused_words_equal"] is True and rec["baby_steps"] > 1, rec
