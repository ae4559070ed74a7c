"""-m gpu: plaintext addition on residues on the device (include/dpfhe.h dpfhe_add_plain, csrc/k_plain_add.hip).

The kernel must give the host twin's words (tests/test_add_plain_cpu.py holds the host twin to Python integers) at N = 256 - fewer than 256 lanes per
polynomial, one partial workgroup per item - and at N = 4096 - eight workgroups per item -, on one and three fold limbs and on the all-class mixture of
tests/class_edges.py, for a broadcast, a grouped and a one-to-one plaintext, with 2 and 3 components, in place and out of place, with the wrap-edge
sums of the CPU test planted in every item; and in the NTT domain: on the transformed operands the entry gives the twin's words on them, and their
inverse transform is the coefficient-domain result (the addition commutes with the transform).  arena_cases() is the footprint case, and - run again by
tests/test_gpu_stream_contract_add_plain.py with Case.gate set - the stream-contract case."""
import numpy as np
import pytest

import test_gpu_footprint as fp
from class_edges import Rig, edge_chain, edge_moduli
from deeppowers_amd import _cabi
from test_add_plain_cpu import operands, twin
from test_seeded_cpu import SENTINEL

pytestmark = pytest.mark.gpu

CONTEXTS = [(kind, ln) for ln in (8, 12) for kind in ("fold1", "fold3", "mixed")]
BATCH = 6


def params(kind, log2n):
    return edge_moduli("mixed", log2n) if kind == "mixed" else edge_chain("fold", log2n, int(kind[4:]))


@pytest.fixture
def rig():
    made = []

    def make(kind, log2n):
        r = Rig(params(kind, log2n))
        r.kind = kind
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=fp.ids(CONTEXTS))
def test_device_matches_host_twin(rig, kind, log2n):
    import torch
    from deeppowers_amd.evaluator import to_host
    r = rig(kind, log2n)
    p, lib, h = r.p, r.ctx._lib, r.ctx.handle
    assert len(set(r.ctx.limb_classes)) == (5 if kind == "mixed" else 1)
    rng = np.random.default_rng(log2n)
    for comps in (2, 3):
        for items in (1, 2, BATCH):
            ct, plain = operands(rng, p, BATCH, comps, items)
            for negate in (False, True):
                want = twin(p, ct, plain, negate)
                what = (kind, log2n, comps, items, negate)
                # coefficient domain, in place (the Python mirror) and out of place into a sentinel-filled buffer
                d_plain = r.dev(plain)
                d_ct = r.ev.add_plain_(r.dev(ct), d_plain, negate)
                d_in = r.dev(ct)
                d_out = torch.full_like(d_in, int(SENTINEL.view(np.int64)))
                _cabi.check(lib.dpfhe_add_plain(h, d_out.data_ptr(), d_in.data_ptr(), d_plain.data_ptr(), BATCH, comps, items, int(negate), None), "dpfhe_add_plain")
                torch.cuda.synchronize()
                assert np.array_equal(to_host(d_ct), want), what
                assert np.array_equal(to_host(d_out), want), what
                assert np.array_equal(to_host(d_in), ct), what                 # the input of the out-of-place call is untouched
                # NTT domain: the same entry on the transformed operands gives the twin's words on them, and the transform of the words above
                n_ct, n_plain = r.ev.ntt_forward(r.dev(ct)), r.ev.ntt_forward(r.dev(plain))
                h_ct, h_plain = to_host(n_ct), to_host(n_plain)
                n_out = torch.full_like(n_ct, int(SENTINEL.view(np.int64)))
                _cabi.check(lib.dpfhe_add_plain(h, n_out.data_ptr(), n_ct.data_ptr(), n_plain.data_ptr(), BATCH, comps, items, int(negate), None), "dpfhe_add_plain")
                r.ev.add_plain_(n_ct, n_plain, negate)
                torch.cuda.synchronize()
                want_ntt = twin(p, h_ct, h_plain, negate)
                assert np.array_equal(to_host(n_ct), want_ntt) and np.array_equal(to_host(n_out), want_ntt), what
                assert np.array_equal(to_host(r.ev.ntt_inverse(n_out)), want), what


def arena_cases(r):
    """out of place (3 components, two plaintext items for four ciphertexts, subtraction) and in place (2 components, one-to-one, addition): every buffer
    carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item"""
    p, lib, h, L, n = r.p, r.ctx._lib, r.ctx.handle, r.L, r.n
    rng = np.random.default_rng(r.n)
    ct, plain = operands(rng, p, 4, 3, 2)
    c = fp.Case(r)
    c.inp("in", ct, 3 * L * n)
    c.inp("plain", plain, L * n)
    c.out("out", ct.size, 3 * L * n, twin(p, ct, plain, negate=True))
    c.run("dpfhe_add_plain, out of place", lambda at: lib.dpfhe_add_plain(h, at("out"), at("in"), at("plain"), 4, 3, 2, 1, at.stream))
    ct, plain = operands(rng, p, 3, 2, 3)
    c = fp.Case(r)
    c.inout("ct", ct, 2 * L * n, twin(p, ct, plain))
    c.inp("plain", plain, L * n)
    c.run("dpfhe_add_plain, in place", lambda at: lib.dpfhe_add_plain(h, at("ct"), at("ct"), at("plain"), 3, 2, 3, 0, at.stream))


def test_footprint(rig):
    assert fp.Case.gate is None
    arena_cases(rig("mixed", 8))


def test_device_entry_rejects_bad_arguments(rig):
    import torch
    r = rig("fold3", 12)
    p, lib, h = r.p, r.ctx._lib, r.ctx.handle
    ct = torch.zeros((9, 2, p.n_limbs, p.n), dtype=torch.int64, device=r.ctx.device)
    pl = torch.ones((2, p.n_limbs, p.n), dtype=torch.int64, device=r.ctx.device)
    c, q, item = ct.data_ptr(), pl.data_ptr(), 2 * p.n_limbs * p.n * 8
    assert lib.dpfhe_add_plain(None, c, c, q, 4, 2, 2, 0, None) == 2000
    for args in ((None, c, q, 4, 2, 2), (c, None, q, 4, 2, 2), (c, c, None, 4, 2, 2), (c, c, q, 4, 1, 2), (c, c, q, 4, 4, 2), (c, c, q, 0, 2, 2),
                 (c, c, q, 3, 2, 2), (c, c, q, 4, 2, 0), (c + 8, c + 8, q, 4, 2, 2), (c, c, q + 8, 4, 2, 2), (c + 4 * item + 8, c, q, 4, 2, 2),
                 (c + item, c, q, 4, 2, 2), (q, q, q, 2, 2, 2), (c, c, q, 1 << 29, 2, 1)):
        assert lib.dpfhe_add_plain(h, *args, 0, None) == 2000, args
    with pytest.raises(_cabi.DpfheError):
        r.ev.add_plain_(ct, pl[:, :, :16].contiguous())
    with pytest.raises(_cabi.DpfheError):
        r.ev.add_plain_(ct, pl[0])
    torch.cuda.synchronize()
    assert int(ct.abs().sum()) == 0
    assert lib.dpfhe_add_plain(h, c + 4 * item, c, q, 4, 2, 2, 0, None) == 0     # apart, aligned: accepted
    torch.cuda.synchronize()
    assert int(ct[4:8, 0].sum()) == 4 * p.n_limbs * p.n and int(ct[:4].abs().sum()) == 0 and int(ct[4:8, 1].abs().sum()) == 0 and int(ct[8].abs().sum()) == 0
