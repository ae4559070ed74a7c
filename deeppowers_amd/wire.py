"""Ciphertext wire format - the Python twin of PolyBuffer::save/load in
include/deeppowers/fhe.hpp.  Little-endian: b"DPFHEv1\0", u32 log2_n, u32 n_limbs, u64 batch, u64 components,
u32 is_ntt, u32 reserved, u64 moduli[n_limbs], then the u64 words [batch][component][limb][N].

Seeded streams (DPFHEs1, the twin of PolyBuffer::save_seeded / load_seeded): one component - the uniform c1 of a fresh symmetric
ciphertext, the a_j of a key - is not sent but re-expanded from a public 32-byte seed (include/dpfhe.h dpfhe_expand_uniform).
Header, 80 bytes, little-endian: b"DPFHEs1\0", u32 log2_n, u32 n_limbs, u64 batch, u64 components, u32 is_ntt,
u32 expanded_component, u64 first_item, u8 seed[32]; then u64 moduli[n_limbs]; then the words of every OTHER component,
[batch][components - 1][L][N].  Size = 80 + 8 L + 8 batch (components - 1) L N.  A seed must never be reused under one secret key.

Compact result streams (DPFHEc1, the twin of CompactCiphertext::save / load): 2-component results switched from Q to 2^k_c and bit-packed
(include/dpfhe.h dpfhe_compact).  32-byte header: b"DPFHEc1\0", u32 log2_n, u32 bits0, u32 bits1, u32 reserved = 0, u64 batch; then the records,
N (bits0 + bits1) / 8 bytes each.  loads / loads_seeded reject them (another magic)."""
from __future__ import annotations

import struct

import numpy as np

from .params import FheParams

MAGIC = b"DPFHEv1\0"
_HDR = struct.Struct("<8sIIQQII")


def dumps(words: np.ndarray, params: FheParams, is_ntt: bool) -> bytes:
    """words: uint64 array shaped [batch][components][L][N] (canonical residues)."""
    a = np.ascontiguousarray(words, dtype="<u8")
    if a.ndim != 4 or a.shape[2] != params.n_limbs or a.shape[3] != params.n:
        raise ValueError("words must be [batch][components][L][N]")
    q = np.array(params.moduli, dtype=np.uint64)[None, None, :, None]
    if (a >= q).any():
        raise ValueError("non-canonical residue")
    hdr = _HDR.pack(MAGIC, params.log2_n, params.n_limbs, a.shape[0], a.shape[1], 1 if is_ntt else 0, 0)
    return hdr + np.array(params.moduli, dtype="<u8").tobytes() + a.tobytes()


def loads(blob: bytes, params: FheParams):
    """-> (words [batch][components][L][N] uint64, is_ntt).  Raises ValueError on any mismatch with `params`."""
    if len(blob) < _HDR.size:
        raise ValueError("truncated header")
    magic, log2_n, n_limbs, batch, comps, is_ntt, _ = _HDR.unpack_from(blob, 0)
    if magic != MAGIC:
        raise ValueError("not a DPFHEv1 stream")
    if log2_n != params.log2_n or n_limbs != params.n_limbs:
        raise ValueError("header does not match the parameters")
    off = _HDR.size
    moduli = np.frombuffer(blob, dtype="<u8", count=n_limbs, offset=off)
    if tuple(int(m) for m in moduli) != tuple(params.moduli):
        raise ValueError("moduli differ")
    off += 8 * n_limbs
    count = batch * comps * n_limbs * params.n
    if len(blob) != off + 8 * count:
        raise ValueError("payload size does not match the header")
    words = np.frombuffer(blob, dtype="<u8", count=count, offset=off).reshape(batch, comps, n_limbs, params.n).astype(np.uint64)
    if (words >= np.array(params.moduli, dtype=np.uint64)[None, None, :, None]).any():
        raise ValueError("non-canonical residue")
    return words, bool(is_ntt)


SEEDED_MAGIC = b"DPFHEs1\0"
_SHDR = struct.Struct("<8sIIQQIIQ32s")


def expand_host(params: FheParams, batch: int, components: int, component: int, seed: bytes, first_item: int = 0,
                out: np.ndarray | None = None) -> np.ndarray:
    """Host twin of dpfhe_expand_uniform: component `component` of items 0 .. batch-1 of `out` ([batch][components][L][N] uint64, zeros when
    None) = expand(seed, first_item + b, limb, component); the other words are left as they are."""
    import ctypes as C

    from . import _cabi
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes")
    if not (0 <= component < components) or first_item < 0 or first_item + batch > 1 << 32:
        raise ValueError("component must be < components and first_item + batch <= 2^32")
    if out is None:
        out = np.zeros((batch, components, params.n_limbs, params.n), dtype=np.uint64)
    if out.dtype != np.uint64 or not out.flags.c_contiguous or out.shape != (batch, components, params.n_limbs, params.n):
        raise ValueError("out must be a contiguous uint64 array [batch][components][L][N]")
    lib = _cabi.load()
    m = (C.c_uint64 * params.n_limbs)(*params.moduli)
    _cabi.check(lib.dpfhe_expand_uniform_host(m, params.n_limbs, params.log2_n, out.ctypes.data, batch, components, component, seed, first_item),
                "dpfhe_expand_uniform_host")
    return out


def noise_host(params: FheParams, batch: int, components: int, component: int, kind: int, param: int, stream_id: int, seed: bytes,
               first_item: int = 0, add: bool = False, out: np.ndarray | None = None) -> np.ndarray:
    """Host twin of dpfhe_sample_noise (include/dpfhe.h): component `component` of items 0 .. batch-1 of `out` ([batch][components][L][N] uint64,
    zeros when None) = noise(seed, first_item + b, stream_id, kind, param), or += it mod q with add; the other words are left as they are.
    kind 0 ternary, 1 centred binomial (eta = 21), 2 flood on [-2^param, 2^param).  The seed is SECRET and serves one call only."""
    import ctypes as C

    from . import _cabi
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes")
    if not (0 <= component < components) or batch < 1 or first_item < 0 or first_item + batch > 1 << 32 or not (0 <= stream_id < 1 << 32):
        raise ValueError("component must be < components, batch >= 1, first_item + batch <= 2^32, stream_id a u32")
    if kind not in (0, 1, 2) or (kind == 2 and not (1 <= param <= 250)):
        raise ValueError("kind 0, 1 or 2; flood bits in [1, 250]")
    if out is None:
        out = np.zeros((batch, components, params.n_limbs, params.n), dtype=np.uint64)
    if out.dtype != np.uint64 or not out.flags.c_contiguous or out.shape != (batch, components, params.n_limbs, params.n):
        raise ValueError("out must be a contiguous uint64 array [batch][components][L][N]")
    lib = _cabi.load()
    m = (C.c_uint64 * params.n_limbs)(*params.moduli)
    _cabi.check(lib.dpfhe_sample_noise_host(m, params.n_limbs, params.log2_n, out.ctypes.data, batch, components, component, kind, int(param) if kind == 2 else 0,
                                            stream_id, seed, first_item, _cabi.NOISE_ADD if add else 0), "dpfhe_sample_noise_host")
    return out


def dumps_seeded(words: np.ndarray, params: FheParams, is_ntt: bool, seed: bytes, component: int = 1, first_item: int = 0,
                 verify: bool = True) -> bytes:
    """words: uint64 [batch][components][L][N] whose component `component` is expand(seed, first_item + b, ., component).  That component is
    left out of the stream; with verify=True it is checked against the host twin first (a stale seed raises ValueError)."""
    a = np.ascontiguousarray(words, dtype="<u8")
    if a.ndim != 4 or a.shape[2] != params.n_limbs or a.shape[3] != params.n:
        raise ValueError("words must be [batch][components][L][N]")
    batch, comps = a.shape[:2]
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes")
    if not (0 <= component < comps) or first_item < 0 or first_item + batch > 1 << 32:
        raise ValueError("component must be < components and first_item + batch <= 2^32")
    q = np.array(params.moduli, dtype=np.uint64)[None, None, :, None]
    if (a >= q).any():
        raise ValueError("non-canonical residue")
    if verify:
        exp = np.zeros((batch, comps, params.n_limbs, params.n), dtype=np.uint64)
        expand_host(params, batch, comps, component, seed, first_item, out=exp)
        if not np.array_equal(exp[:, component], a[:, component]):
            raise ValueError("component does not match its seed (overwritten, transformed or another seed)")
    stored = np.ascontiguousarray(np.delete(a, component, axis=1), dtype="<u8")
    hdr = _SHDR.pack(SEEDED_MAGIC, params.log2_n, params.n_limbs, batch, comps, 1 if is_ntt else 0, component, first_item, seed)
    return hdr + np.array(params.moduli, dtype="<u8").tobytes() + stored.tobytes()


def loads_seeded(blob: bytes, params: FheParams):
    """-> (stored words [batch][components - 1][L][N] uint64, is_ntt, seed, component, first_item).  Raises ValueError on any mismatch."""
    if len(blob) < _SHDR.size:
        raise ValueError("truncated header")
    magic, log2_n, n_limbs, batch, comps, is_ntt, component, first_item, seed = _SHDR.unpack_from(blob, 0)
    if magic != SEEDED_MAGIC:
        raise ValueError("not a DPFHEs1 stream")
    if log2_n != params.log2_n or n_limbs != params.n_limbs:
        raise ValueError("header does not match the parameters")
    if component >= comps:
        raise ValueError("expanded_component must be < components")
    if first_item + batch > 1 << 32:
        raise ValueError("first_item + batch must be <= 2^32")
    off = _SHDR.size
    if len(blob) < off + 8 * n_limbs:
        raise ValueError("truncated moduli")
    moduli = np.frombuffer(blob, dtype="<u8", count=n_limbs, offset=off)
    if tuple(int(m) for m in moduli) != tuple(params.moduli):
        raise ValueError("moduli differ")
    off += 8 * n_limbs
    count = batch * (comps - 1) * n_limbs * params.n
    if len(blob) != off + 8 * count:
        raise ValueError("payload size does not match the header")
    words = np.frombuffer(blob, dtype="<u8", count=count, offset=off).reshape(batch, comps - 1, n_limbs, params.n).astype(np.uint64)
    if (words >= np.array(params.moduli, dtype=np.uint64)[None, None, :, None]).any():
        raise ValueError("non-canonical residue")
    return words, bool(is_ntt), bytes(seed), int(component), int(first_item)


def inflate_seeded(stored: np.ndarray, params: FheParams, seed: bytes, component: int, first_item: int = 0) -> np.ndarray:
    """stored words [batch][components - 1][L][N] (loads_seeded) -> the full words [batch][components][L][N], the missing component
    expanded by the host twin (clients without a GPU, host-only servers)."""
    batch, kept = stored.shape[:2]
    full = np.empty((batch, kept + 1, params.n_limbs, params.n), dtype=np.uint64)
    full[:, :component] = stored[:, :component]
    full[:, component + 1:] = stored[:, component:]
    return expand_host(params, batch, kept + 1, component, seed, first_item, out=full)


COMPACT_MAGIC = b"DPFHEc1\0"
_CHDR = struct.Struct("<8sIIIIQ")


def compact_bits(log2_n: int, t: int) -> tuple[int, int]:
    """Recommended widths (k_0, k_1) of a compact result (Evaluator.compact, DPFHEc1) for plaintext modulus t at N = 2^log2_n:
    k_0 = ceil(log2 t) + 2, k_1 = ceil(log2 t + 3 + log2 sqrt(N ln(2^65) / 2)).  The c0 rounding costs at most 1/8 of the decryption tolerance, the
    c1 rounding times the ternary secret at most 1/8 with probability >= 1 - 2^-64 per coefficient (Hoeffding over <= N terms), so any ciphertext
    with a noise budget of at least 2 bits still decrypts.  Both widths are at least 8; ValueError if one would exceed 60."""
    import math
    if not (8 <= log2_n <= 16) or not (2 <= t < 1 << 32):
        raise ValueError("log2_n in [8, 16] and t in [2, 2^32)")
    lt = math.log2(t)
    k0 = max(8, math.ceil(lt) + 2)
    k1 = max(8, math.ceil(lt + 3 + math.log2(math.sqrt((1 << log2_n) * math.log(2.0 ** 65) / 2))))
    if k1 > 60:
        raise ValueError("width above 60 bits")
    return k0, k1


def compact_record_bytes(log2_n: int, bits0: int, bits1: int) -> int:
    return ((bits0 + bits1) << log2_n) // 8


def dumps_compact(records: np.ndarray, log2_n: int, bits0: int, bits1: int) -> bytes:
    """records: uint8 [batch][N (bits0 + bits1) / 8] (Evaluator.compact, dpfhe_compact_host).  32-byte little-endian header: b"DPFHEc1\\0",
    u32 log2_n, u32 bits0, u32 bits1, u32 reserved = 0, u64 batch; then the records.  Size = 32 + batch N (bits0 + bits1) / 8."""
    a = np.ascontiguousarray(records, dtype=np.uint8)
    if not (8 <= log2_n <= 16) or not (8 <= bits0 <= 60) or not (8 <= bits1 <= 60):
        raise ValueError("log2_n in [8, 16] and widths in [8, 60]")
    if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] != compact_record_bytes(log2_n, bits0, bits1):
        raise ValueError("records must be [batch][N (bits0 + bits1) / 8] with batch >= 1")
    return _CHDR.pack(COMPACT_MAGIC, log2_n, bits0, bits1, 0, a.shape[0]) + a.tobytes()


def loads_compact(blob: bytes):
    """-> (records uint8 [batch][N (bits0 + bits1) / 8], log2_n, bits0, bits1).  Raises ValueError on a bad header or a wrong size."""
    if len(blob) < _CHDR.size:
        raise ValueError("truncated header")
    magic, log2_n, bits0, bits1, reserved, batch = _CHDR.unpack_from(blob, 0)
    if magic != COMPACT_MAGIC:
        raise ValueError("not a DPFHEc1 stream")
    if reserved != 0 or not (8 <= log2_n <= 16) or not (8 <= bits0 <= 60) or not (8 <= bits1 <= 60) or batch == 0:
        raise ValueError("bad header")
    rec = compact_record_bytes(log2_n, bits0, bits1)
    if len(blob) != _CHDR.size + batch * rec:
        raise ValueError("payload size does not match the header")
    return np.frombuffer(blob, dtype=np.uint8, offset=_CHDR.size).reshape(batch, rec).copy(), int(log2_n), int(bits0), int(bits1)


def compact_host(params: FheParams, words: np.ndarray, bits0: int, bits1: int) -> np.ndarray:
    """Host twin of Evaluator.compact / dpfhe_compact: words uint64 [batch][2][L][N] -> records uint8 [batch][N (bits0 + bits1) / 8]."""
    import ctypes as C

    from . import _cabi
    a = np.ascontiguousarray(words, dtype=np.uint64)
    if a.ndim != 4 or a.shape[1] != 2 or a.shape[2] != params.n_limbs or a.shape[3] != params.n:
        raise ValueError("words must be [batch][2][L][N]")
    out = np.empty((a.shape[0], compact_record_bytes(params.log2_n, bits0, bits1)), dtype=np.uint8)
    lib = _cabi.load()
    m = (C.c_uint64 * params.n_limbs)(*params.moduli)
    _cabi.check(lib.dpfhe_compact_host(m, params.n_limbs, params.log2_n, out.ctypes.data, a.ctypes.data, a.shape[0], bits0, bits1), "dpfhe_compact_host")
    return out
