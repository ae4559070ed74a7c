"""Complex slot encoding on the host (include/dpfhe.h "complex slot encoding"): what a client needs on its side of the approximate (CKKS-style)
family, over dpfhe_encode_complex_host and dpfhe_decode_complex_host.  No device, no context."""
import ctypes as C

import numpy as np

from . import _cabi


def aligned(shape, dtype):
    """a zeroed C-contiguous array whose data is 16-byte aligned (the entries take 16-byte loads and stores)"""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    raw = np.zeros(count * dtype.itemsize + 16, dtype=np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + count * dtype.itemsize].view(dtype).reshape(shape)


def _slots(slots, log2_n):
    slots = np.asarray(slots)
    real = not np.iscomplexobj(slots)
    if slots.ndim != 2 or slots.shape[0] == 0 or slots.shape[1] != (1 << log2_n) // 2:
        raise _cabi.DpfheError(2000, "slots: a non-empty [items][N/2] array")
    buf = aligned(slots.shape, np.float64 if real else np.complex128)
    buf[...] = slots
    return buf, real


def encode_host(slots, scale, log2_n, moduli=None):
    """slots [items][N/2], complex or real -> round(scale m): int64 [items][N] (moduli None: what Encryptor.encrypt takes), or uint64 [items][L][N]
    canonical residues on `moduli`"""
    buf, real = _slots(slots, log2_n)
    items, n = buf.shape[0], 1 << log2_n
    flags = _cabi.ENCODE_REAL if real else 0
    if moduli is None:
        mods, flags, out = (3,), flags | _cabi.ENCODE_PLAIN, aligned((items, n), np.uint64)
    else:
        mods, out = tuple(int(q) for q in moduli), aligned((items, len(moduli), n), np.uint64)
    m = (C.c_uint64 * len(mods))(*mods)
    _cabi.check(_cabi.load().dpfhe_encode_complex_host(m, len(mods), log2_n, out.ctypes.data, buf.ctypes.data, items, float(scale), flags),
                "dpfhe_encode_complex_host")
    return out.view(np.int64) if moduli is None else out


def decode_host(coeffs, scale, log2_n, real=False):
    """centred int64 coefficients [items][N] -> the slots m(xi^(3^i)) / scale: complex128 [items][N/2], or float64 real parts"""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int64)
    n = 1 << log2_n
    if coeffs.ndim != 2 or coeffs.shape[0] == 0 or coeffs.shape[1] != n:
        raise _cabi.DpfheError(2000, "coeffs: a non-empty [items][N] array")
    out = np.zeros((coeffs.shape[0], n // 2), dtype=np.float64 if real else np.complex128)
    _cabi.check(_cabi.load().dpfhe_decode_complex_host(log2_n, out.ctypes.data, coeffs.ctypes.data, coeffs.shape[0], float(scale),
                                                       _cabi.ENCODE_REAL if real else 0), "dpfhe_decode_complex_host")
    return out
