"""CPU: noise polynomials for re-randomised results (include/dpfhe.h dpfhe_sample_noise_host, wire.noise_host).

noise(seed, item, stream_id, kind, param) is restated here from its definition with Python integers - the ChaCha20 block function of
tests/test_seeded_cpu.py (checked there against RFC 8439 and openssl), one 256-bit little-endian X per coefficient, the three maps X -> v, and
v mod q by Python's own % - and the library's host twin must give the same words.  The device kernel is held to the host twin by
tests/test_gpu_rerandomize.py."""
import ctypes as C

import numpy as np
import pytest

from deeppowers_amd import _cabi, wire
from deeppowers_amd.params import FheParams, ntt_primes
from test_seeded_cpu import SEED, chacha20_blocks_np, mixed_params, pinned60, primes31

TERNARY, CBD21, FLOOD = 0, 1, 2
FLOOD_BITS = (1, 2, 63, 64, 100, 127, 128, 200, 250)
FIRST_ITEMS = (0, (1 << 31) + 5)
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
DOMAIN = 0x6B73616D


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def noise_ints(seed: bytes, item: int, stream_id: int, kind: int, param: int, n: int) -> np.ndarray:
    """the N signed integers v_k of noise(seed, item, stream_id, kind, param), as Python integers in an object array"""
    w = chacha20_blocks_np(seed, np.arange(n // 2, dtype=np.uint32), (item, stream_id, DOMAIN)).astype(object).reshape(n, 8)
    xs = [sum(int(w[k, i]) << (32 * i) for i in range(8)) for k in range(n)]
    if kind == TERNARY:
        v = [(3 * (x % (1 << 64))) // (1 << 64) - 1 for x in xs]
    elif kind == CBD21:
        v = [bin(x & 0x1FFFFF).count("1") - bin((x >> 21) & 0x1FFFFF).count("1") for x in xs]
    else:
        v = [x % (1 << (param + 1)) - (1 << param) for x in xs]
    return np.array(v, dtype=object)


def noise_ref(p: FheParams, batch, comps, comp, kind, param, stream_id, seed, first_item, add=False, fill=None) -> np.ndarray:
    out = np.zeros((batch, comps, p.n_limbs, p.n), dtype=np.uint64) if fill is None else fill.copy()
    for b in range(batch):
        v = noise_ints(seed, first_item + b, stream_id, kind, param, p.n)
        for l, q in enumerate(p.moduli):
            r = np.array([int(x) % q for x in v], dtype=np.uint64)         # Python's % is the canonical residue of a negative value too
            out[b, comp, l] = (out[b, comp, l] + r) % np.uint64(q) if add else r   # both below 2^60: no wrap
    return out


def _fills(p, batch, comps, rng):
    q = np.array(p.moduli, dtype=np.uint64)[None, None, :, None]
    shape = (batch, comps, p.n_limbs, p.n)
    return {"set": (False, np.full(shape, SENTINEL, dtype=np.uint64)),
            "add_random": (True, rng.integers(0, 2**62, shape, dtype=np.uint64) % q),
            "add_qm1": (True, np.broadcast_to(q - np.uint64(1), shape).copy())}


def _check(p, batch, comps, comp, kind, param, stream_id, first_item, modes=("set", "add_random", "add_qm1"), seed=SEED):
    rng = np.random.default_rng(1000 * kind + param)
    fills = _fills(p, batch, comps, rng)
    others = [c for c in range(comps) if c != comp]
    base = noise_ref(p, batch, comps, comp, kind, param, stream_id, seed, first_item)
    q = np.array(p.moduli, dtype=np.uint64)[None, :, None]
    for mode in modes:
        add, fill = fills[mode]
        if others:
            fill[:, others] = SENTINEL
        got = wire.noise_host(p, batch, comps, comp, kind, param, stream_id, seed, first_item, add=add, out=fill.copy())
        want = fill.copy()
        want[:, comp] = (fill[:, comp] + base[:, comp]) % q if add else base[:, comp]
        assert np.array_equal(got, want), (p.log2_n, p.moduli, kind, param, first_item, mode)
        assert (got[:, others] == SENTINEL).all()                          # every other component untouched
        assert (got[:, comp] < q).all()


# ---- 1: host twin == restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", range(8, 17))
def test_host_twin_matches_restatement_every_ring_degree(log2n):
    p = ntt_primes(log2n, 2 if log2n <= 12 else 1, 60)
    batch = 2 if log2n <= 10 else 1
    modes = ("set", "add_random", "add_qm1")
    for i, kind in enumerate((TERNARY, CBD21)):
        _check(p, batch, 2, i, kind, 0, 7 + i, FIRST_ITEMS[(log2n + i) % 2], modes=modes if log2n <= 12 else modes[i::2])
    for i, f in enumerate(FLOOD_BITS):
        _check(p, 1, 3, i % 3, FLOOD, f, 2, FIRST_ITEMS[i % 2], modes=(modes[(i + log2n) % 3],) if log2n >= 12 else modes)


@pytest.mark.parametrize("name", ["pinned60", "primes31", "mixed", "config1"])
def test_host_twin_matches_restatement_parameter_sets(name):
    p = {"pinned60": pinned60, "primes31": primes31, "mixed": mixed_params, "config1": FheParams.config1}[name]()
    for first in FIRST_ITEMS:
        _check(p, 2, 2, 1, TERNARY, 0, 0, first)
        _check(p, 2, 3, 0, CBD21, 0, 1, first)
        for f in FLOOD_BITS:
            _check(p, 1, 2, 0, FLOOD, f, 2, first)


def test_host_twin_matches_restatement_on_the_smallest_primes():
    """every limb a smallest prime = 1 mod 2N (class_edges 'smallest'): q below 2^18, so a flood value of 64 or 250 bits is reduced from far above q -
    what tests/test_gpu_rerandomize.py's comparison at the catalogue's extremes rests on"""
    from class_edges import edge_moduli
    for log2n in (8, 12):
        p = edge_moduli("smallest", log2n)
        assert max(p.moduli) < 1 << 18
        first = FIRST_ITEMS[log2n % 2]
        _check(p, 2, 2, 1, TERNARY, 0, 0, first)
        _check(p, 2, 3, 0, CBD21, 0, 1, first)
        for f in (1, 64, 250):
            _check(p, 1, 2, 0, FLOOD, f, 2, first)


def test_more_limbs_than_one_launch_group():
    p = ntt_primes(8, 19, 60)                                              # the limb constants travel 16 limbs at a time
    _check(p, 2, 2, 1, FLOOD, 200, 2, 3)
    _check(p, 1, 2, 0, CBD21, 0, 1, 0, modes=("add_random",))


# ---- 2: one integer on every limb ------------------------------------------------------------------------------------------------
def _crt_centred(p: FheParams, rows: np.ndarray) -> np.ndarray:
    """rows [L][n] canonical residues -> the integers in (-Q/2, Q/2) they represent (object array)"""
    Q = 1
    for q in p.moduli:
        Q *= q
    acc = np.zeros(rows.shape[1], dtype=object)
    for l, q in enumerate(p.moduli):
        m = Q // q
        acc = acc + rows[l].astype(object) * (m * pow(m, -1, q))
    acc = acc % Q
    return np.where(acc > Q // 2, acc - Q, acc)


@pytest.mark.parametrize("kind,f", [(TERNARY, 0), (CBD21, 0)] + [(FLOOD, f) for f in FLOOD_BITS])
def test_every_limb_holds_the_same_integer(kind, f):
    p = ntt_primes(10, 5, 60)                                              # Q > 2^295 > 2^(250 + 2)
    got = wire.noise_host(p, 2, 2, 1, kind, f, 2, SEED, 9)
    for b in range(2):
        assert np.array_equal(_crt_centred(p, got[b, 1]), noise_ints(SEED, 9 + b, 2, kind, f, p.n))
    m = mixed_params(10)                                                   # 60 + 40 + 59 + 54 + 49 = 262 bits
    if f + 2 < 258:
        got = wire.noise_host(m, 1, 1, 0, kind, f, 0, SEED)
        assert np.array_equal(_crt_centred(m, got[0, 0]), noise_ints(SEED, 0, 0, kind, f, m.n))


# ---- 3: streams ------------------------------------------------------------------------------------------------------------------
def test_first_item_selects_the_range_of_a_larger_batch():
    p = primes31(10, 2)
    for kind, f in ((TERNARY, 0), (CBD21, 0), (FLOOD, 40)):
        whole = wire.noise_host(p, 8, 2, 1, kind, f, 3, SEED, 0)
        assert np.array_equal(whole[5:], wire.noise_host(p, 3, 2, 1, kind, f, 3, SEED, 5))


def test_streams_items_seeds_and_expand_are_unrelated():
    p = ntt_primes(16, 1, 60)
    base = wire.noise_host(p, 1, 1, 0, FLOOD, 58, 2, SEED)[0, 0, 0]
    for other in (wire.noise_host(p, 1, 1, 0, FLOOD, 58, 1, SEED)[0, 0, 0], wire.noise_host(p, 1, 1, 0, FLOOD, 58, 2, SEED, 1)[0, 0, 0],
                  wire.noise_host(p, 1, 1, 0, FLOOD, 58, 2, bytes(32))[0, 0, 0]):
        assert np.count_nonzero(base == other) < 8
    # one seed misused for both formats: the raw 128-bit halves of the noise words differ from expand's words of every component
    # (flood at f = 58 keeps the low 59 bits of X; compare them with the low bits of what expand reduces)
    for comp in range(3):
        for stream_id in range(3):
            e = wire.expand_host(p, 1, 3, comp, SEED)[0, comp, 0]
            nz = wire.noise_host(p, 1, 1, 0, FLOOD, 58, stream_id, SEED)[0, 0, 0]
            assert np.count_nonzero(e == nz) < 8
    # the same block serves both coefficients of a pair, but they are different words of it
    assert np.count_nonzero(base[0::2] == base[1::2]) < 8


# ---- 4: distributions (deterministic: the seed is fixed) -------------------------------------------------------------------------
def _centred_one_limb(p, words):
    q = p.moduli[0]
    w = words.astype(np.int64)
    return np.where(w > q // 2, w - q, w)


def test_ternary_distribution():
    p = ntt_primes(16, 1, 60)
    v = _centred_one_limb(p, wire.noise_host(p, 16, 1, 0, TERNARY, 0, 0, SEED)[:, 0, 0].reshape(-1))
    assert v.size == 1 << 20 and set(np.unique(v)) == {-1, 0, 1}
    sigma = np.sqrt(v.size * (1 / 3) * (2 / 3))
    for x in (-1, 0, 1):
        dev = (np.count_nonzero(v == x) - v.size / 3) / sigma
        print("ternary", x, "deviation", round(float(dev), 2), "sigma")
        assert abs(dev) < 5


def test_cbd21_distribution():
    p = ntt_primes(16, 1, 60)
    v = _centred_one_limb(p, wire.noise_host(p, 16, 1, 0, CBD21, 0, 1, SEED)[:, 0, 0].reshape(-1)).astype(np.float64)
    n = v.size
    assert n == 1 << 20 and np.abs(v).max() <= 21
    var = 10.5                                                             # 42 fair bits, each of variance 1/4
    mean_dev = v.mean() / np.sqrt(var / n)
    # the sample variance has variance (mu4 - var^2) / n; a sum of 42 independent +-1/2: mu4 = 42 / 16 + 3 * 42 * 41 / 16 = 3 var^2 - 42 / 8
    mu4 = 3 * var * var - 42 / 8
    var_dev = (v.var() - var) / np.sqrt((mu4 - var * var) / n)
    print("cbd mean", round(float(mean_dev), 2), "sigma; variance", round(float(v.var()), 4), round(float(var_dev), 2), "sigma; max", np.abs(v).max())
    assert abs(mean_dev) < 5 and abs(var_dev) < 5


@pytest.mark.parametrize("f", FLOOD_BITS)
def test_flood_distribution(f):
    limbs = (f + 2) // 59 + 1                                              # Q > 2^(59 limbs) > 2^(f + 2)
    p = ntt_primes(16, limbs, 60)
    words = wire.noise_host(p, 16, 1, 0, FLOOD, f, 2, SEED)[:, 0]          # [16][L][N]
    rows = np.ascontiguousarray(words.transpose(1, 0, 2)).reshape(limbs, -1)
    v = _centred_one_limb(p, rows[0]).astype(object) if limbs == 1 else _crt_centred(p, rows)
    assert v.size == 1 << 20
    lo, hi = -(1 << f), 1 << f
    assert min(v) >= lo and max(v) < hi
    assert max(abs(x) for x in v) >= 1 << (f - 1)
    top_bits = min(4, f + 1)                                               # f = 1, 2 have fewer than four bits: all of them
    cells = np.array([(int(x) - lo) >> (f + 1 - top_bits) for x in v], dtype=np.int64)
    counts = np.bincount(cells, minlength=1 << top_bits)
    expected = v.size / (1 << top_bits)
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("flood", f, "chi-square", round(chi2, 1))
    assert chi2 < 60, chi2


# ---- 5: argument checks ----------------------------------------------------------------------------------------------------------
def test_c_entries_reject_bad_arguments_and_write_nothing():
    lib = _cabi.load()
    p = primes31(8, 2)
    m = (C.c_uint64 * 2)(*p.moduli)
    out = np.full((2, 2, 2, p.n), SENTINEL, dtype=np.uint64)
    o = out.ctypes.data
    ok = (m, 2, 8, o, 2, 2, 1, FLOOD, 20, 0, SEED, 0, 0)
    bad = {
        "null moduli": (None,) + ok[1:],
        "no limbs": ok[:1] + (0,) + ok[2:],
        "log2_n 7": ok[:2] + (7,) + ok[3:],
        "log2_n 17": ok[:2] + (17,) + ok[3:],
        "null out": ok[:3] + (None,) + ok[4:],
        "batch 0": ok[:4] + (0,) + ok[5:],
        "comp = comps": ok[:6] + (2,) + ok[7:],
        "kind 3": ok[:7] + (3,) + ok[8:],
        "f = 0": ok[:8] + (0,) + ok[9:],
        "f = 251": ok[:8] + (251,) + ok[9:],
        "null seed": ok[:10] + (None,) + ok[11:],
        "first_item + batch > 2^32": ok[:11] + (0xFFFFFFFF,) + ok[12:],
        "unknown flag": ok[:12] + (2,),
    }
    for why, args in bad.items():
        assert lib.dpfhe_sample_noise_host(*args) == 2000, why
    even = (C.c_uint64 * 2)(p.moduli[0], 1 << 40)
    assert lib.dpfhe_sample_noise_host(even, *ok[1:]) == 2000
    assert (out == SENTINEL).all()
    assert lib.dpfhe_sample_noise_host(*ok) == 0 and (out[:, 0] == SENTINEL).all() and (out[:, 1] != SENTINEL).all()
    # the device entries refuse a null context before anything else
    assert lib.dpfhe_sample_noise(None, o, 2, 2, 1, FLOOD, 20, 0, SEED, 0, 0, None) == 2000
    assert lib.dpfhe_rerandomize(None, o, o, 1, 20, SEED, 0, o, None) == 2000
    # the Python mirror's own checks
    for kw in (dict(seed=b"short"), dict(component=2), dict(kind=3), dict(param=0), dict(param=251), dict(first_item=1 << 32), dict(batch=0)):
        a = dict(batch=2, components=2, component=1, kind=FLOOD, param=20, stream_id=0, seed=SEED, first_item=0)
        a.update(kw)
        with pytest.raises(ValueError):
            wire.noise_host(p, **a)
