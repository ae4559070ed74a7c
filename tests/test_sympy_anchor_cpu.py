"""CPU: tests/golden/sympy_anchor.json - words that sympy alone produced at the metric rings (make_golden.py sympy_anchor) - against everything on the
host that claims the same words: the big-int oracle (the functions it has), oracle.c (every family) and the thread-by-thread emulator of the kernels'
own code (transforms in every form, the fused multiply's data paths).  The fixture's cheap sections are generated again here with every pyoracle
function but SplitMix64 disabled: the file matches its generator, and the generator does not lean on the oracle."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import sympy_anchor as sa
from class_edges import expected_class
from oracle import pyoracle as po
from oracle.cbind import Oracle
from test_emulated_kernels import GENERIC, HALVES, ONE_PIECE, QUARTERS, emu  # noqa: F401  (the fixture that builds tools/libemu.so)

U = C.POINTER(C.c_uint64)
ARITH = {"shoup": 0, "fold": 1, "f64": 2, "fold_scaled": 3, "f64_wide": 4}
ALL_TRANSFORMS = [r for ln in sa.TRANSFORM_LOG2NS for r in sa.transform_records(ln)]
MULTIPLY = sa.fixture()["multiply"]
tid = lambda r: "%s-n%d-%s-%s" % (r["name"], 1 << r["log2n"], r.get("direction", "mul"), r["input"])
p64 = lambda a: a.ctypes.data_as(U)


def test_inputs_are_the_generators():
    """the numpy restatement of splitmix64 and of the input layouts (tests/sympy_anchor.py, what the GPU test draws from) against oracle/pyoracle.py's"""
    g = po.SplitMix64(12345)
    assert [int(v) for v in sa.splitmix_words(12345, 100)] == [g.next() for _ in range(100)]
    qs = [(1 << 60) - 93, 1073707009, 65537]
    g = po.SplitMix64((1 << 63) + 7)
    assert sa.fill("random", (1 << 63) + 7, qs, 64).tolist() == [g.words_mod(64, q) for q in qs]
    mg = _generator()
    for kind in ("random", "qm1", "monomial"):
        assert sa.fill(kind, 9, qs, 16).ravel().tolist() == mg.anchor_fill(kind, 9, qs, 16)
    for length, pos in sa.fixture()["positions"].items():
        assert pos == mg.anchor_positions(int(length)) and len(set(pos)) == 32


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_for_anchor", os.path.join(os.path.dirname(sa.GOLDEN), "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_has_every_section_and_stays_small():
    fx = sa.fixture()
    names = lambda ln: [r["name"] for r in sa.transform_records(ln) if r["input"] == "random" and r["direction"] == "fwd"]
    classes = ["fold", "f64", "fold_scaled", "f64_wide", "shoup"]
    assert names(12) == classes + ["pinned0", "pinned1", "pinned2", "pinned3"] and names(13) == names(12)
    assert names(14) == ["pinned1", "pinned2", "pinned4"] and names(15) == ["pinned4", "shoup"] and names(16) == names(15)
    for ln in (12, 13):
        for r in sa.transform_records(ln)[:5]:
            assert expected_class(r["q"]) == r["name"]
    assert {(r["name"], r["input"], r["direction"]) for r in sa.transform_records(12)} >= {(c, k, d) for c in classes for k in ("qm1", "monomial") for d in ("fwd", "inv")}
    assert [r["name"] for r in MULTIPLY] == ["config1_n1024", "metric_n4096_pair0", "metric_n4096_pair1", "metric_n4096_extremes", "mixed_n4096", "n8192_pinned_f64"]
    assert [expected_class(q).split("_")[0] for q in MULTIPLY[4]["moduli"]] == ["fold", "fold", "f64", "f64"] and [q.bit_length() for q in MULTIPLY[4]["moduli"]] == [59, 50, 40, 33]
    assert [(c["op"], c["input"]) for c in fx["integer"]["cases"]] == [(op, k) for k in ("random", "qm1") for op in ("rescale", "base_extend", "scale_round")]
    assert [(c["op"], c["input"]) for c in fx["keyswitch"]["cases"]] == [(op, k) for k in ("random", "qm1") for op in ("relinearize", "switch_key_hybrid")]
    golden = os.path.dirname(sa.GOLDEN)
    others = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f.endswith(".json") and f != "sympy_anchor.json"]
    assert os.path.getsize(sa.GOLDEN) < max(others)


def test_cheap_sections_regenerate_without_the_oracle(monkeypatch):
    """the transforms at log2 N = 12 and the integer operations, generated again with every pyoracle function other than SplitMix64 replaced by one that
    raises: equal to the committed file"""
    mg = _generator()

    def refuse(name):
        def raiser(*a, **k):
            raise AssertionError("the anchor generator called oracle.pyoracle.%s" % name)
        return raiser
    for name, obj in list(vars(mg.po).items()):
        if callable(obj) and not name.startswith("__") and name != "SplitMix64" and getattr(obj, "__module__", None) == mg.po.__name__:
            monkeypatch.setattr(mg.po, name, refuse(name))
    with pytest.raises(AssertionError):
        mg.po.ntt_forward([1, 2], 17, 4)
    again = mg.sympy_anchor(only=mg.ANCHOR_CHEAP)
    fx = sa.fixture()
    assert set(mg.ANCHOR_CHEAP) <= set(again)
    for section in mg.ANCHOR_CHEAP:
        assert again[section] == fx[section], section
    for length, pos in again["positions"].items():
        assert fx["positions"][length] == pos


# ---- transforms ---------------------------------------------------------------------------------------------------------------------------------------
def _transform_input(r):
    return sa.fill(r["input"], r["seed"], [r["q"]], 1 << r["log2n"])[0]


@pytest.mark.parametrize("r", ALL_TRANSFORMS, ids=tid)
def test_both_oracles_reproduce_the_transform_anchors(r):
    n = 1 << r["log2n"]
    a = _transform_input(r)
    orc = Oracle(r["log2n"], [r["q"]], [r["psi"]])
    sa.assert_anchor(r, (orc.ntt_fwd if r["direction"] == "fwd" else orc.ntt_inv)(a), n, "oracle.c")
    f = po.ntt_forward if r["direction"] == "fwd" else po.ntt_inverse
    sa.assert_anchor(r, np.array(f(a.tolist(), r["q"], r["psi"]), np.uint64), n, "pyoracle")


def _emu_contexts(log2n):
    """(moduli, psis, forms, the records of each limb): the contexts the emulator runs the anchored primes in - the five class primes as ONE context
    (per-limb classes, what ntt_classes_kernel launches), the pinned primes as one fold context in every form it has at that ring degree (one-piece or
    split, halves at 8192, quarters at 16384, and the generic tables), the generic prime of 2^15 / 2^16 alone"""
    recs = sa.transform_records(log2n)
    by_name = {}
    for r in recs:
        by_name.setdefault(r["name"], []).append(r)
    groups = []
    cls = [nm for nm in by_name if not nm.startswith("pinned") and log2n <= 13]
    if cls:
        groups.append((cls, (ONE_PIECE, GENERIC)))
    pinned = [nm for nm in by_name if nm.startswith("pinned")]
    groups.append((pinned, (ONE_PIECE, GENERIC) + {13: (HALVES,), 14: (QUARTERS,)}.get(log2n, ())))
    if log2n >= 15:
        groups.append((["shoup"], (ONE_PIECE,)))
    for names, forms in groups:
        yield [by_name[nm][0]["q"] for nm in names], [by_name[nm][0]["psi"] for nm in names], forms, [by_name[nm] for nm in names]


@pytest.mark.parametrize("log2n", sa.TRANSFORM_LOG2NS)
def test_emulated_transforms_reproduce_the_anchors_in_every_form(emu, log2n):  # noqa: F811
    n = 1 << log2n
    emu.emu_ctx_ntt.argtypes = [C.c_int, C.c_int, U, U, C.c_int, C.c_int, C.c_int, U, U]
    emu.emu_ctx_ntt.restype = C.c_int
    before = emu.emu_overflows()
    ran = set()
    for qs, psis, forms, limbs in _emu_contexts(log2n):
        m, w = np.array(qs, np.uint64), np.array(psis, np.uint64)
        for limb, recs in enumerate(limbs):
            for r in recs:
                a = np.ascontiguousarray(_transform_input(r))
                for form in forms:
                    out = np.zeros_like(a)
                    assert emu.emu_ctx_ntt(log2n, len(qs), p64(m), p64(w), limb, form, int(r["direction"] == "inv"), p64(a), p64(out)) == 0, (r["name"], form)
                    sa.assert_anchor(r, out, n, "emu_ctx_ntt form %d" % form)
                    ran.add(form)
    assert ran >= {ONE_PIECE, GENERIC} | {13: {HALVES}, 14: {QUARTERS}}.get(log2n, set())
    assert emu.emu_overflows() == before, "lazy arithmetic wrapped around 2^64"


# ---- the tensor product ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", MULTIPLY, ids=tid)
def test_both_oracles_reproduce_the_multiply_anchors(r):
    n, L = 1 << r["log2n"], len(r["moduli"])
    a, b = sa.multiply_operands(r)
    orc = Oracle(r["log2n"], r["moduli"], r["psi"])
    c = orc.ct_mul(a[None], b[None], threads=0)[0]
    sa.assert_anchor(r, c, n, "oracle.c")
    want = po.ct_mul_ntt(a.tolist(), b.tolist(), r["moduli"], r["psi"])
    sa.assert_anchor(r, np.array(want, np.uint64), n, "pyoracle")
    if "ntt_a" in r:
        for key, x in (("ntt_a", a), ("ntt_b", b), ("ntt_c", c)):
            sa.assert_anchor(r[key], orc.ntt_fwd(x, threads=0), n, "oracle.c " + key)
            got = [[po.ntt_forward(x[comp][l].tolist(), r["moduli"][l], r["psi"][l]) for l in range(L)] for comp in range(x.shape[0])]
            sa.assert_anchor(r[key], np.array(got, np.uint64), n, "pyoracle " + key)


@pytest.mark.parametrize("r", MULTIPLY, ids=tid)
def test_emulated_fused_multiply_reproduces_the_anchors(emu, r):  # noqa: F811
    """every data path the emulator has for a limb's class: emu_ct_mul_lazy_class (the lazy products of the quad / dual kernels: every class but shoup),
    emu_ct_mul_class (the generic path through canonical words: every class but fold) and, on the fold limbs of N = 4096, emu_ct_mul_lazy29
    (ct_mul_quad_kernel as shipped), with coefficient-domain output and - where the product's transform is anchored - with NTT-domain output"""
    n, L, log2n = 1 << r["log2n"], len(r["moduli"]), r["log2n"]
    for fn in (emu.emu_ct_mul_lazy_class, emu.emu_ct_mul_class):
        fn.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, U, U, U, U, U]
        fn.restype = C.c_int
    emu.emu_ct_mul_lazy29.argtypes = [C.c_uint64, C.c_uint64, C.c_int, U, U, U, U, U]
    emu.emu_ct_mul_lazy29.restype = C.c_int
    before = emu.emu_overflows()
    a, b = sa.multiply_operands(r)
    ran = set()
    for l, (q, psi) in enumerate(zip(r["moduli"], r["psi"])):
        cls = expected_class(q)
        ops = [np.ascontiguousarray(v) for v in (a[0, l], a[1, l], b[0, l], b[1, l])]
        paths = []
        if cls != "shoup":
            paths.append(("lazy_class", r, lambda o: emu.emu_ct_mul_lazy_class(ARITH[cls], log2n, q, psi, *map(p64, ops), p64(o))))
        if cls != "fold":
            paths.append(("class", r, lambda o: emu.emu_ct_mul_class(ARITH[cls], log2n, q, psi, *map(p64, ops), p64(o))))
        if cls == "fold" and log2n == 12:
            paths.append(("lazy29", r, lambda o: emu.emu_ct_mul_lazy29(q, psi, 0, *map(p64, ops), p64(o))))
            if "ntt_c" in r:
                paths.append(("lazy29_ntt", r["ntt_c"], lambda o: emu.emu_ct_mul_lazy29(q, psi, 1, *map(p64, ops), p64(o))))
        assert paths
        for path, rec, call in paths:
            out = np.zeros(3 * n, np.uint64)
            assert call(out) == 0, (path, l)
            for comp in range(3):      # one limb at a time: the anchor's digest of that polynomial
                assert sa.digest(out[comp * n:(comp + 1) * n]) == rec["poly_sha256"][comp * L + l], (r["name"], path, "component", comp, "limb", l)
            ran.add(path)
    if all(expected_class(q) == "fold" for q in r["moduli"]) and log2n == 12:
        assert ran == {"lazy_class", "lazy29"} | ({"lazy29_ntt"} if "ntt_c" in r else set())
    assert emu.emu_overflows() == before, "a lazy-arithmetic precondition was broken"


# ---- integer operations -----------------------------------------------------------------------------------------------------------------------------------
def _integer_input(fx, c):
    return sa.fill(c["input"], c["seed"], fx["moduli"], 1 << fx["log2n"])


@pytest.mark.parametrize("c", sa.fixture()["integer"]["cases"], ids=lambda c: c["op"] + "-" + c["input"])
def test_both_oracles_reproduce_the_integer_anchors(c):
    fx = sa.fixture()["integer"]
    n, moduli = 1 << fx["log2n"], fx["moduli"]
    x = _integer_input(fx, c)
    orc = Oracle(fx["log2n"], moduli, fx["psi"])
    if c["op"] == "rescale":
        by_c = orc.rescale(x)
        by_py = po.scale_round(x.tolist(), moduli, [3], [0, 1, 2], 1)          # (pyoracle has no rescale of its own: the same rounding with multiplier 1)
    elif c["op"] == "base_extend":
        by_c = orc.base_extend(x[c["src_limb0"]:c["src_limb0"] + c["n_src"]], c["src_limb0"], c["dst_limb0"], c["n_dst"])
        by_py = po.base_extend(x[:c["n_src"]].tolist(), moduli[:c["n_src"]], moduli[c["dst_limb0"]:c["dst_limb0"] + c["n_dst"]])
    else:
        by_c = orc.scale_round(x, c["drop_limb0"], c["n_drop"], c["keep_limb0"], c["n_keep"], c["multiplier"])
        by_py = po.scale_round(x.tolist(), moduli, list(range(c["drop_limb0"], c["drop_limb0"] + c["n_drop"])),
                               list(range(c["keep_limb0"], c["keep_limb0"] + c["n_keep"])), c["multiplier"])
    sa.assert_anchor(c, by_c, n, "oracle.c")
    sa.assert_anchor(c, np.array(by_py, np.uint64), n, "pyoracle")


# ---- key switching ----------------------------------------------------------------------------------------------------------------------------------------
def keyswitch_inputs(fx, c):
    """(ciphertext, key) of a key-switching anchor: relinearize [3][L][N] and [L][2][L][N]; switch_key_hybrid [2][L-1][N] and [L-1][2][L][N]"""
    n, moduli = 1 << fx["log2n"], fx["moduli"]
    L = len(moduli)
    if c["op"] == "relinearize":
        return sa.fill(c["input"], c["seed"], moduli * 3, n).reshape(3, L, n), sa.fill("random", c["key_seed"], sa.key_moduli(moduli, L), n).reshape(L, 2, L, n)
    return sa.fill(c["input"], c["seed"], moduli[:L - 1] * 2, n).reshape(2, L - 1, n), sa.fill("random", c["key_seed"], sa.key_moduli(moduli, L - 1), n).reshape(L - 1, 2, L, n)


@pytest.mark.parametrize("c", sa.fixture()["keyswitch"]["cases"], ids=lambda c: c["op"] + "-" + c["input"])
def test_oracle_c_reproduces_the_key_switching_anchors(c):
    fx = sa.fixture()["keyswitch"]
    orc = Oracle(fx["log2n"], fx["moduli"], fx["psi"])
    ct, key = keyswitch_inputs(fx, c)
    got = orc.relinearize(ct[None], key, threads=0) if c["op"] == "relinearize" else orc.keyswitch_hybrid(ct[None], key, 2, threads=0)
    sa.assert_anchor(c, got, 1 << fx["log2n"], "oracle.c")


# ---- the Galois identity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", [12, 16])
def test_oracle_c_galois_map_satisfies_the_evaluation_identity(log2n):
    """(sigma_g a)(rho) = a(rho^g) at 32 sampled rho = psi^odd, g in {3, 5, N + 1, 2N - 1}: oracle.c's orc_apply_galois, and the identity's own power to
    tell a wrong map (a different g, a dropped sign) from the right one"""
    n = 1 << log2n
    for r in (r for r in sa.transform_records(log2n) if r["direction"] == "fwd" and r["input"] == "random" and (log2n == 12 or r["name"] == "pinned4")):
        a = _transform_input(r)
        orc = Oracle(log2n, [r["q"]], [r["psi"]])
        for g in sa.galois_elements(n):
            rotated = orc.apply_galois(a[None, None], g).ravel()
            assert sa.galois_identity_failures(a, rotated, g, r["q"], r["psi"], 77 + g) == [], (r["name"], g)
        if log2n == 12 and r["name"] == "pinned0":
            wrong = orc.apply_galois(a[None, None], 7).ravel()
            assert len(sa.galois_identity_failures(a, wrong, 3, r["q"], r["psi"], 80)) == sa.GALOIS_POINTS
            flipped = orc.apply_galois(a[None, None], 3).ravel()
            flipped[5] = (r["q"] - int(flipped[5])) % r["q"]
            assert sa.galois_identity_failures(a, flipped, 3, r["q"], r["psi"], 80)
