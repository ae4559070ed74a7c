"""CPU: compact result ciphertexts (include/dpfhe.h dpfhe_compact_host, csrc/compact.h, wire DPFHEc1).

The host twin must give round(2^k X / Q) mod 2^k, bit-packed, computed here with Python integers straight from the definition (not through the
centred-remainder identity the library uses), on every limb class, for 1 to 10 limbs, for widths from 8 to 60 bits, with X at 0, Q - 1 and on both
sides of rounding boundaries.  A hand-written record pins the bit layout.  A toy exact encryption shows that a compact result decrypts at the
recommended widths and not with a narrow c1.  The device kernel is held to the host twin by tests/test_gpu_compact.py."""
import ctypes as C
import math

import numpy as np
import pytest

from deeppowers_amd import _cabi, wire
from deeppowers_amd.params import PRIMES_60, FheParams, ntt_primes
from test_plain_add_cpu import shoup55
from test_rlwe_semantics import encrypt, small_params

WIDTHS = ((8, 8), (19, 28), (17, 29), (13, 41), (60, 60))


def pinned(log2n, count):
    """2^60 - d primes (fold class): the pinned chain, continued by ntt_primes beyond its length"""
    return small_params(log2n, count) if count <= len(PRIMES_60) else ntt_primes(log2n, count, 60)


# the limb classes: fold (pinned 2^60 - d), f64 (< 2^47), f64_wide (< 2^50), fold_scaled (2^k - d0), shoup (generic 55-bit)
CLASSES = {
    "fold": pinned,
    "f64": lambda log2n, L: ntt_primes(log2n, L, 40),
    "f64_wide": lambda log2n, L: ntt_primes(log2n, L, 49),
    "fold_scaled": lambda log2n, L: ntt_primes(log2n, L, 59),
    "shoup": lambda log2n, L: shoup55(log2n, L),
}


def twin(p: FheParams, words: np.ndarray, bits0: int, bits1: int) -> np.ndarray:
    """dpfhe_compact_host: words uint64 [batch][2][L][N] -> records uint8 [batch][N (bits0 + bits1) / 8]"""
    return wire.compact_host(p, words, bits0, bits1)


def pack(values, k: int) -> np.ndarray:
    """value j at bits [j k, (j + 1) k) of a little-endian bit string"""
    v = np.array([int(x) for x in values], dtype=np.uint64)
    bits = ((v[:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def unpack(record: np.ndarray, n: int, k: int) -> np.ndarray:
    bits = np.unpackbits(record, bitorder="little")[: n * k].reshape(n, k).astype(np.uint64)
    return (bits << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def crt_values(p: FheParams, residues: np.ndarray) -> np.ndarray:
    """residues uint64 [L][N] -> object array of X in [0, Q)"""
    Q = math.prod(p.moduli)
    X = np.zeros(p.n, dtype=object)
    for l, q in enumerate(p.moduli):
        Ql = Q // q
        X = X + residues[l].astype(object) * (Ql * pow(Ql, -1, q))
    return X % Q


def reference(p: FheParams, words: np.ndarray, bits0: int, bits1: int) -> np.ndarray:
    """round(2^k X / Q) = floor((2^{k+1} X + Q) / 2 Q) mod 2^k with Python integers (Q odd: no tie), then packed"""
    Q = math.prod(p.moduli)
    out = []
    for item in words:
        rec = []
        for c, k in ((0, bits0), (1, bits1)):
            X = crt_values(p, item[c])
            rec.append(pack(((X * (2 << k) + Q) // (2 * Q)) % (1 << k), k))
        out.append(np.concatenate(rec))
    return np.stack(out)


def residues_of(p: FheParams, xs) -> np.ndarray:
    return np.array([[x % q for x in xs] for q in p.moduli], dtype=np.uint64)


def random_words(rng, p: FheParams, batch) -> np.ndarray:
    """random canonical residues, with 0, Q - 1 and X on both sides of rounding boundaries of both widths planted in item 0"""
    q = np.array(p.moduli, dtype=np.uint64)[None, None, :, None]
    return (rng.integers(0, 1 << 63, (batch, 2, p.n_limbs, p.n), dtype=np.uint64) % q).astype(np.uint64)


def plant_edges(p: FheParams, words: np.ndarray, bits0: int, bits1: int) -> None:
    Q = math.prod(p.moduli)
    for c, k in ((0, bits0), (1, bits1)):
        xs = [0, Q - 1, 1, Q // 2, Q // 2 + 1]
        for a in (0, 1, (1 << (k - 1)) - 1, 1 << (k - 1), (1 << k) - 2, (1 << k) - 1):
            b = (2 * a + 1) * Q >> (k + 1)          # floor((2a+1) Q / 2^{k+1}): rounds to a, b + 1 rounds to a + 1
            xs += [b, b + 1]
        words[0, c, :, : len(xs)] = residues_of(p, xs)


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("L", [1, 2, 3, 4, 6, 10])
def test_host_twin_matches_big_integer_definition(cls, L):
    rng = np.random.default_rng(L * 31 + len(cls))
    for log2n in (8, 12):
        p = CLASSES[cls](log2n, L)
        for bits0, bits1 in WIDTHS:
            words = random_words(rng, p, 2 if log2n == 8 else 1)
            plant_edges(p, words, bits0, bits1)
            assert np.array_equal(twin(p, words, bits0, bits1), reference(p, words, bits0, bits1)), (cls, L, log2n, bits0, bits1)


def test_host_twin_matches_big_integer_definition_on_the_smallest_primes():
    """every limb a smallest prime = 1 mod 2N (class_edges 'smallest': q below 2^18, Q below 2^52 - narrower than the widest record width): what
    tests/test_gpu_compact.py's comparison at the catalogue's extremes rests on"""
    from class_edges import edge_moduli
    rng = np.random.default_rng(77)
    for log2n in (8, 12):
        p = edge_moduli("smallest", log2n)
        assert max(p.moduli) < 1 << 18
        for bits0, bits1 in WIDTHS:
            words = random_words(rng, p, 2)
            plant_edges(p, words, bits0, bits1)
            words[1] = np.array(p.moduli, dtype=np.uint64)[None, :, None] - np.uint64(1)      # X = Q - 1 in every coefficient
            assert np.array_equal(twin(p, words, bits0, bits1), reference(p, words, bits0, bits1)), (log2n, bits0, bits1)


def test_host_twin_largest_ring():
    p = ntt_primes(16, 3, 60)
    rng = np.random.default_rng(16)
    words = random_words(rng, p, 1)
    plant_edges(p, words, 19, 29)
    assert np.array_equal(twin(p, words, 19, 29), reference(p, words, 19, 29))


def test_edges_round_as_defined():
    """the planted values themselves: 0 -> 0, Q - 1 -> 2^k mod 2^k = 0, boundary pairs -> a and a + 1 (mod 2^k)"""
    p = pinned(8, 3)
    Q = math.prod(p.moduli)
    k = 13
    words = np.zeros((1, 2, 3, p.n), dtype=np.uint64)
    a = 1234
    b = (2 * a + 1) * Q >> (k + 1)
    words[0, 0, :, :4] = residues_of(p, [0, Q - 1, b, b + 1])
    got = unpack(twin(p, words, k, k)[0], p.n, k)
    assert [int(v) for v in got[:4]] == [0, 0, a, a + 1]


def test_packing_fixture():
    """N = 256, widths (8, 12), one limb: component 0 holds 0 .. 255 (so its bytes are 0 .. 255), component 1 alternates 0xABC and 0x123
    (each pair is the 24-bit little-endian word 0x123ABC: bytes BC 3A 12)."""
    p = pinned(8, 1)
    q = p.moduli[0]
    # X = ceil(a Q / 2^k) rounds to a (2^k / Q is far below 1/2)
    x_of = lambda a, k: -(-a * q // (1 << k))
    words = np.zeros((1, 2, 1, 256), dtype=np.uint64)
    words[0, 0, 0] = [x_of(j, 8) for j in range(256)]
    words[0, 1, 0] = [x_of(0xABC if j % 2 == 0 else 0x123, 12) for j in range(256)]
    want = bytes(range(256)) + bytes([0xBC, 0x3A, 0x12]) * 128
    got = twin(p, words, 8, 12)
    assert got.shape == (1, 640) and got.tobytes() == want


def test_records_and_items_are_laid_out_back_to_back():
    p = pinned(8, 2)
    rng = np.random.default_rng(5)
    words = random_words(rng, p, 3)
    one = [twin(p, words[i : i + 1], 13, 41) for i in range(3)]
    assert np.array_equal(twin(p, words, 13, 41), np.concatenate(one))
    assert one[0].shape[1] == 256 * (13 + 41) // 8


def test_host_twin_rejects_bad_arguments():
    lib = _cabi.load()
    p = pinned(8, 2)
    n = p.n
    m = (C.c_uint64 * 11)(*ntt_primes(8, 11, 60).moduli)
    words = np.zeros((2, 2, 11, n), dtype=np.uint64)
    out = np.full(2 * n * 120 // 8 + 64, 0xA5, dtype=np.uint8)
    w, o = words.ctypes.data, out.ctypes.data
    good = (m, 2, 8, o, w, 1, 19, 28)

    def call(**kw):
        args = dict(zip(("moduli", "L", "log2n", "out", "inp", "batch", "b0", "b1"), good))
        args.update(kw)
        return lib.dpfhe_compact_host(*args.values())

    bad = [dict(moduli=None), dict(out=None), dict(inp=None), dict(batch=0), dict(log2n=7), dict(log2n=17), dict(L=0), dict(L=11),
           dict(b0=7), dict(b0=61), dict(b1=7), dict(b1=61), dict(b0=0), dict(b1=64), dict(out=w + 8)]
    for kw in bad:
        assert call(**kw) == 2000, kw
    for moduli in ((4, 7), (1, 7), (1 << 60 | 1, 7), (7, 7), (15, 21), (0, 7)):
        mm = (C.c_uint64 * 2)(*moduli)
        assert call(moduli=mm) == 2000, moduli
    # out overlapping the input's last word
    assert call(out=w + 2 * 2 * n * 8 - 8) == 2000
    assert (out == 0xA5).all()                  # nothing was written
    assert call() == 0


def test_compact_bits_values():
    assert wire.compact_bits(11, 65537) == (19, 27)
    assert wire.compact_bits(12, 65537) == (19, 28)
    assert wire.compact_bits(13, 65537) == (19, 28)
    assert wire.compact_bits(14, 65537) == (19, 29)
    assert wire.compact_bits(8, 3) == (8, 11)                  # ceil(log2 3) + 2 = 4 is raised to the minimum width 8
    with pytest.raises(ValueError):
        wire.compact_bits(17, 65537)


def test_stream_round_trip_and_rejections():
    p = pinned(8, 3)
    rng = np.random.default_rng(9)
    recs = twin(p, random_words(rng, p, 3), 19, 28)
    blob = wire.dumps_compact(recs, 8, 19, 28)
    assert len(blob) == 32 + 3 * 256 * (19 + 28) // 8
    assert blob[:8] == b"DPFHEc1\0"
    got, log2_n, b0, b1 = wire.loads_compact(blob)
    assert (log2_n, b0, b1) == (8, 19, 28) and np.array_equal(got, recs)
    for broken in (blob[:-1], blob + b"\0", blob[:20], b"DPFHEv1\0" + blob[8:], blob[:24] + b"\0" * 8 + blob[32:],
                   blob[:20] + (1).to_bytes(4, "little") + blob[24:]):
        with pytest.raises(ValueError):
            wire.loads_compact(broken)
    # the full-word readers keep rejecting it
    with pytest.raises(ValueError):
        wire.loads(blob, p)
    with pytest.raises(ValueError):
        wire.loads_seeded(blob, p)
    with pytest.raises(ValueError):
        wire.dumps_compact(recs[:, :-1], 8, 19, 28)


def decrypt_compact(record: np.ndarray, n: int, s, bits0: int, bits1: int, t: int) -> np.ndarray:
    """phase = c0 2^{K-k0} + (c1 * s) 2^{K-k1} mod 2^K (negacyclic product in wrapping u64), m = round(t phase / 2^K) mod t"""
    K = max(bits0, bits1)
    c0 = unpack(record[: n * bits0 // 8], n, bits0)
    c1 = unpack(record[n * bits0 // 8 :], n, bits1)
    acc = np.zeros(n, dtype=np.uint64)
    for j in np.nonzero(s)[0]:
        sh = np.concatenate([(np.uint64(0) - c1[n - j :]), c1[: n - j]])   # c1 x^j mod X^N + 1
        acc = acc + sh if s[j] > 0 else acc - sh
    mask = (1 << K) - 1
    phase = [((int(a) << (K - bits0)) + (int(b) << (K - bits1))) & mask for a, b in zip(c0, acc)]
    return np.array([((t * ph * 2 + (1 << K)) >> (K + 1)) % t for ph in phase], dtype=np.int64)


def test_exact_encryption_decrypts_from_compact_form():
    """N = 2048, three 60-bit limbs, a fresh exact encryption of random messages mod t = 65537: compact at the recommended widths decrypts every
    coefficient; with k_1 = 17 most coefficients decrypt wrong."""
    p = small_params(11, 3)
    t = 65537
    rng = np.random.default_rng(2048)
    s = rng.integers(-1, 2, p.n)
    msg = rng.integers(0, t, p.n)
    Q = math.prod(p.moduli)
    ct, _ = encrypt(rng, p, s, msg, Q // t)
    bits0, bits1 = wire.compact_bits(11, t)
    assert (bits0, bits1) == (19, 27)
    rec = twin(p, ct[None], bits0, bits1)[0]
    assert np.array_equal(decrypt_compact(rec, p.n, s, bits0, bits1, t), msg)
    narrow = twin(p, ct[None], 19, 17)[0]
    wrong = np.count_nonzero(decrypt_compact(narrow, p.n, s, 19, 17, t) != msg)
    assert wrong > p.n // 2, wrong
