"""CPU: seeded uniform polynomials (include/dpfhe.h dpfhe_expand_uniform_host, wire.py DPFHEs1, rpc.py seeded streams).

expand(seed, item, limb, component) is a wire format, so it is restated here from its definition - the ChaCha20 block function of
RFC 8439 section 2.3 in plain Python (checked against the RFC's vector and against openssl), and the 128-bit reduction with Python
integers - and the library's host twin must give the same words.  The device kernel is held to the host twin by tests/test_gpu_seeded.py."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from deeppowers_amd import _cabi, rpc, wire
from deeppowers_amd.params import FheParams, is_prime, min_primitive_2n_root, ntt_primes

MASK = 0xFFFFFFFF
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)   # "expand 32-byte k"


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _rotl(v, c):
    return ((v << c) & MASK) | (v >> (32 - c))


def chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    """RFC 8439 section 2.3: 64 bytes of key stream for (key, 32-bit counter, 96-bit nonce)"""
    st = list(SIGMA) + list(struct.unpack("<8I", key)) + [counter & MASK] + list(struct.unpack("<3I", nonce))
    x = list(st)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & MASK; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & MASK; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & MASK; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & MASK; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return struct.pack("<16I", *[(x[i] + st[i]) & MASK for i in range(16)])


def chacha20_blocks_np(key: bytes, counters: np.ndarray, nonce_words) -> np.ndarray:
    """the same block function over many counters at once (numpy uint32, wrapping arithmetic) -> [len(counters)][16] words"""
    n = len(counters)
    st = [np.full(n, v, dtype=np.uint32) for v in SIGMA + struct.unpack("<8I", key)]
    st += [counters.astype(np.uint32)] + [np.full(n, v, dtype=np.uint32) for v in nonce_words]
    x = [v.copy() for v in st]

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return np.stack([x[i] + st[i] for i in range(16)], axis=1)


def expand_ref(seed: bytes, item: int, limb: int, comp: int, q: int, n: int) -> np.ndarray:
    """expand(seed, item, limb, component) mod q: block k / 4, words 4 (k mod 4) .. +3 as one little-endian 128-bit X, X % q"""
    w = chacha20_blocks_np(seed, np.arange(n // 4, dtype=np.uint32), (item, limb, comp)).astype(object).reshape(n, 4)
    x = w[:, 0] | (w[:, 1] << 32) | (w[:, 2] << 64) | (w[:, 3] << 96)
    return np.array([int(v) % q for v in x], dtype=np.uint64)


def ref_full(p: FheParams, batch, comps, comp, seed, first_item, fill=None):
    out = np.zeros((batch, comps, p.n_limbs, p.n), dtype=np.uint64) if fill is None else fill.copy()
    for b in range(batch):
        for l, q in enumerate(p.moduli):
            out[b, comp, l] = expand_ref(seed, first_item + b, l, comp, q, p.n)
    return out


# ---- parameter sets ------------------------------------------------------------------------------------------------------------
def _shoup_prime(log2n, bits):
    """a prime = 1 mod 2N of `bits` (51 ... 59) bits far from 2^bits: the generic (Shoup) limb class"""
    n = 1 << log2n
    q = (1 << bits) - ((1 << bits) - 1) % (2 * n)
    while True:
        if is_prime(q) and q >= (1 << 50) and (((1 << bits) - q) << (60 - bits)) >= (1 << 24):
            return q, min_primitive_2n_root(n, q)
        q -= 2 * n


def mixed_params(log2n=12):
    """one limb of each class, widths 60 / 40 / 59 / -54 / 49 (fold, f64, fold_scaled, shoup, f64_wide): tests/test_gpu_limb_classes.py"""
    qs, ps = [], []
    for w in (60, 40, 59, None, 49):
        if w is None:
            q, r = _shoup_prime(log2n, 54)
        else:
            p = ntt_primes(log2n, 1, w)
            q, r = p.moduli[0], p.psi[0]
        qs.append(q)
        ps.append(r)
    return FheParams(log2n, tuple(qs), tuple(ps))


def pinned60():
    return FheParams.n4096_l4()


def primes31(log2n=12, count=3):
    return ntt_primes(log2n, count, 31)


SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
SEED = bytes(range(100, 132))


# ---- ChaCha20 ------------------------------------------------------------------------------------------------------------------
def test_rfc8439_block_vector(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "chacha20_rfc8439.json")))
    got = chacha20_block(bytes.fromhex(g["key"]), g["counter"], bytes.fromhex(g["nonce"]))
    assert got.hex() == g["block"] and g["block"].startswith("10f1e7e4d13b5915") and g["block"].endswith("a2503c4e")
    np_words = chacha20_blocks_np(bytes.fromhex(g["key"]), np.array([g["counter"]], dtype=np.uint32),
                                  struct.unpack("<3I", bytes.fromhex(g["nonce"])))
    assert np_words[0].astype("<u4").tobytes() == got


def test_chacha20_matches_openssl_and_numpy_twin():
    rng = np.random.default_rng(8439)
    have_openssl = shutil.which("openssl") is not None
    for _ in range(6):
        key, nonce = rng.bytes(32), rng.bytes(12)
        counter = int(rng.integers(0, 2**32 - 3))
        ref = b"".join(chacha20_block(key, counter + i, nonce) for i in range(3))
        tw = chacha20_blocks_np(key, np.arange(counter, counter + 3, dtype=np.uint64).astype(np.uint32), struct.unpack("<3I", nonce))
        assert tw.astype("<u4").tobytes() == ref
        if have_openssl:   # openssl's -iv for chacha20 = 32-bit little-endian counter || 96-bit nonce; encrypting zeros yields the key stream
            iv = counter.to_bytes(4, "little") + nonce
            out = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex()], input=bytes(192), capture_output=True, check=True).stdout
            assert out == ref
    if not have_openssl:
        pytest.skip("openssl binary absent: RFC vector and numpy twin checked, openssl comparison skipped")


# ---- host twin == restatement ---------------------------------------------------------------------------------------------------
def _check(p, batch, comps, comp, first_item, seed=SEED):
    fill = np.full((batch, comps, p.n_limbs, p.n), SENTINEL, dtype=np.uint64)
    got = wire.expand_host(p, batch, comps, comp, seed, first_item, out=fill.copy())
    want = ref_full(p, batch, comps, comp, seed, first_item, fill=fill)
    assert np.array_equal(got, want), (p.log2_n, p.moduli, comp, first_item)
    others = [c for c in range(comps) if c != comp]
    assert (got[:, others] == SENTINEL).all()                       # every other word untouched
    assert (got[:, comp] < np.array(p.moduli, dtype=np.uint64)[None, :, None]).all()


@pytest.mark.parametrize("log2n", range(8, 17))
def test_host_twin_matches_restatement_every_ring_degree(log2n):
    p = ntt_primes(log2n, 2 if log2n <= 13 else 1, 60)
    _check(p, 2 if log2n <= 12 else 1, 2, 1, 0)
    _check(p, 1, 3, 0 if log2n % 2 else 2, (1 << 31) + 5)


@pytest.mark.parametrize("name", ["pinned60", "primes31", "mixed", "config1"])
def test_host_twin_matches_restatement_limb_classes(name):
    p = {"pinned60": pinned60, "primes31": primes31, "mixed": mixed_params, "config1": FheParams.config1}[name]()
    for comps, comp, first in ((2, 1, 0), (3, 0, (1 << 31) + 5), (3, 2, 7)):
        _check(p, 2, comps, comp, first)


def test_host_twin_matches_restatement_on_the_smallest_primes():
    """every limb a smallest prime = 1 mod 2N (class_edges 'smallest'): a 128-bit X reduced into a q below 2^18 - what tests/test_gpu_seeded.py's
    comparison at the catalogue's extremes rests on"""
    from class_edges import edge_moduli
    for log2n in (8, 12):
        p = edge_moduli("smallest", log2n)
        assert max(p.moduli) < 1 << 18
        for comps, comp, first in ((2, 1, 0), (3, 0, (1 << 31) + 5)):
            _check(p, 2, comps, comp, first)


def test_prefix_property_on_a_dropped_limb_level():
    full = ntt_primes(12, 4, 60)
    lower = full.drop_last_limb()
    a = wire.expand_host(full, 3, 2, 1, SEED, 11)
    b = wire.expand_host(lower, 3, 2, 1, SEED, 11)
    assert np.array_equal(a[:, :, : lower.n_limbs], b)
    m = mixed_params()
    assert np.array_equal(wire.expand_host(m, 1, 2, 1, SEED)[:, :, :3], wire.expand_host(m.drop_last_limb().drop_last_limb(), 1, 2, 1, SEED))


def test_first_item_selects_the_range_of_a_larger_batch():
    p = primes31(10, 2)
    whole = wire.expand_host(p, 8, 2, 1, SEED, 0)
    assert np.array_equal(whole[5:], wire.expand_host(p, 3, 2, 1, SEED, 5))


# ---- statistics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [60, 31])
def test_uniformity_sanity(bits):
    p = ntt_primes(16, 1, bits)
    q = p.moduli[0]
    w = wire.expand_host(p, 16, 2, 1, SEED)[:, 1].reshape(-1)   # 2^20 words
    assert w.size == 1 << 20 and (w < np.uint64(q)).all()
    u = w.astype(np.float64) / q
    sigma = np.sqrt(1 / 12 / u.size)
    assert abs(u.mean() - 0.5) < 5 * sigma
    counts = np.bincount(np.minimum((u * 16).astype(np.int64), 15), minlength=16)
    expected = u.size / 16
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    assert chi2 < 60, chi2                                          # 15 degrees of freedom: p < 1e-6 beyond ~ 50
    # distinct (item, limb, component) streams and seeds give unrelated words
    base = wire.expand_host(p, 1, 3, 1, SEED)[0, 1, 0]
    for other in (wire.expand_host(p, 1, 3, 1, SEED, 1)[0, 1, 0], wire.expand_host(p, 1, 3, 2, SEED)[0, 2, 0],
                  wire.expand_host(p, 1, 3, 1, bytes(32))[0, 1, 0]):
        assert np.count_nonzero(base == other) < 8
    two = ntt_primes(16, 2, bits)
    lim = wire.expand_host(two, 1, 2, 1, SEED)[0, 1]
    assert np.count_nonzero(lim[0] % np.uint64(1 << 20) == lim[1] % np.uint64(1 << 20)) < 64


# ---- DPFHEs1 -------------------------------------------------------------------------------------------------------------------
def _seeded_words(p, batch=3, comps=2, comp=1, first=0, seed=SEED, rng_seed=1):
    rng = np.random.default_rng(rng_seed)
    q = np.array(p.moduli, dtype=np.uint64)[None, None, :, None]
    w = rng.integers(0, 2**62, (batch, comps, p.n_limbs, p.n), dtype=np.uint64) % q
    return wire.expand_host(p, batch, comps, comp, seed, first, out=w)


def test_seeded_roundtrip_layout_and_size():
    p = pinned60()
    for comps, comp, first in ((2, 1, 0), (3, 0, 9), (3, 2, (1 << 31) + 5)):
        w = _seeded_words(p, 3, comps, comp, first)
        blob = wire.dumps_seeded(w, p, True, SEED, component=comp, first_item=first)
        L, n = p.n_limbs, p.n
        assert len(blob) == 80 + 8 * L + 8 * 3 * (comps - 1) * L * n
        assert blob[:8] == b"DPFHEs1\0"
        assert struct.unpack_from("<IIQQIIQ", blob, 8) == (p.log2_n, L, 3, comps, 1, comp, first) and blob[48:80] == SEED
        assert int.from_bytes(blob[80:88], "little") == p.moduli[0]
        stored, is_ntt, seed, c, f = wire.loads_seeded(blob, p)
        assert is_ntt and seed == SEED and (c, f) == (comp, first)
        assert np.array_equal(stored, np.delete(w, comp, axis=1))
        assert np.array_equal(wire.inflate_seeded(stored, p, seed, c, f), w)
    # a seeded two-component ciphertext is (just over) half of its v1 stream
    w = _seeded_words(p, 4)
    assert len(wire.dumps_seeded(w, p, False, SEED)) < 0.501 * len(wire.dumps(w, p, False))


def test_seeded_rejections():
    p = pinned60()
    w = _seeded_words(p, 2)
    blob = wire.dumps_seeded(w, p, False, SEED)
    for bad in (blob[:79], blob[:-8], blob + b"\0" * 8, b"X" + blob[1:]):
        with pytest.raises(ValueError):
            wire.loads_seeded(bad, p)
    with pytest.raises(ValueError):
        wire.loads_seeded(blob, FheParams.config1())
    with pytest.raises(ValueError, match="not a DPFHEv1"):
        wire.loads(blob, p)                                           # v1 readers keep rejecting the new magic
    with pytest.raises(ValueError, match="not a DPFHEs1"):
        wire.loads_seeded(wire.dumps(w, p, False), p)

    def patched(off, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, value)
        return bytes(b)
    with pytest.raises(ValueError, match="expanded_component"):
        wire.loads_seeded(patched(36, "<I", 2), p)                    # expanded_component == components
    with pytest.raises(ValueError, match="2\\^32"):
        wire.loads_seeded(patched(40, "<Q", (1 << 32) - 1), p)        # first_item + batch > 2^32
    with pytest.raises(ValueError, match="moduli"):
        wire.loads_seeded(patched(80, "<Q", p.moduli[0] - 2), p)
    with pytest.raises(ValueError, match="non-canonical"):
        wire.loads_seeded(patched(len(blob) - 8, "<Q", p.moduli[-1]), p)
    # writer side: a wrong or stale seed is caught by verify=True, and nothing else than a valid component is accepted
    with pytest.raises(ValueError, match="seed"):
        wire.dumps_seeded(w, p, False, bytes(32))
    stale = w.copy(); stale[1, 1, 2, 7] ^= np.uint64(1)
    with pytest.raises(ValueError, match="seed"):
        wire.dumps_seeded(stale, p, False, SEED)
    assert wire.dumps_seeded(stale, p, False, SEED, verify=False)    # the caller's responsibility when not verified
    with pytest.raises(ValueError):
        wire.dumps_seeded(w, p, False, SEED, component=2)
    with pytest.raises(ValueError):
        wire.dumps_seeded(w, p, False, SEED[:31])
    with pytest.raises(ValueError):
        wire.dumps_seeded(w, p, False, SEED, first_item=(1 << 32) - 1)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_entries_reject_bad_arguments():
    lib = _cabi.load()
    p = pinned60()
    m = (C.c_uint64 * 4)(*p.moduli)
    out = np.zeros((1, 2, 4, p.n), dtype=np.uint64)
    ptr = out.ctypes.data
    assert lib.dpfhe_expand_uniform(None, ptr, 1, 2, 1, SEED, 0, None) == 2000
    assert lib.dpfhe_expand_uniform_host(None, 4, 12, ptr, 1, 2, 1, SEED, 0) == 2000          # null moduli
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, None, 1, 2, 1, SEED, 0) == 2000            # null output
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, ptr, 1, 2, 1, None, 0) == 2000             # null seed
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, ptr, 1, 2, 2, SEED, 0) == 2000             # component >= components
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, ptr, 1, 0, 0, SEED, 0) == 2000
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, ptr, 1, 2, 1, SEED, 1 << 32) == 2000       # first_item + batch > 2^32
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, ptr, 2, 2, 1, SEED, (1 << 32) - 1) == 2000
    assert lib.dpfhe_expand_uniform_host(m, 4, 7, ptr, 1, 2, 1, SEED, 0) == 2000              # log2_n out of range
    assert lib.dpfhe_expand_uniform_host((C.c_uint64 * 1)(1 << 60), 1, 12, ptr, 1, 2, 1, SEED, 0) == 2000
    assert (out == 0).all()
    assert lib.dpfhe_expand_uniform_host(m, 4, 12, ptr, 1, 2, 1, SEED, (1 << 32) - 1) == 0    # the last item is legal
    assert np.array_equal(out, ref_full(p, 1, 2, 1, SEED, (1 << 32) - 1))


# ---- RPC without a device ------------------------------------------------------------------------------------------------------
def test_seeded_echo_over_rpc_without_a_device():
    p = pinned60()
    server = rpc.EncryptedInferenceServer(None, params=p)
    server.register_model("echo", rpc.Passthrough())
    port = server.start("127.0.0.1:0")
    client = rpc.EncryptedClient(f"127.0.0.1:{port}", p)
    try:
        w = _seeded_words(p, 5, rng_seed=4)
        y, is_ntt = client.generate("echo", w, seed_a=SEED)
        assert not is_ntt and np.array_equal(y, w)
        with pytest.raises(Exception):
            client.generate("echo", w, seed_a=bytes(32))              # the client's own verify catches a wrong seed before sending
    finally:
        client.close()
        server.stop()
