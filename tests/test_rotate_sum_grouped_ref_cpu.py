"""CPU: tests/rotate_sum_grouped_ref.py with one rotation is tests/switch_key_grouped_ref.py (the pinned reference of dpfhe_switch_key_grouped) on the rotated
input, plus the input - the header's n_rot = 1 identity, in Python integers."""
import numpy as np

import rotate_sum_grouped_ref as rs
import switch_key_grouped_ref as ks
from deeppowers_amd.params import ntt_primes
from oracle.cbind import Oracle


def test_one_rotation_is_the_grouped_key_switch_of_the_rotated_input_plus_the_input():
    Ld, alpha, g = 5, 2, 3 * 3 * 3
    p = ntt_primes(8, Ld + alpha)
    orc, data = Oracle.from_params(p), Oracle(8, p.moduli[:Ld], p.psi[:Ld])
    ct, key, at = data.fill(2, 5), orc.fill(3 * 2, 6).reshape(1, 3, 2, Ld + alpha, 256), list(range(256))
    got = rs.divide_and_add(rs.sum_qp(orc, data, ct, [g], key, Ld, alpha), ct, p.moduli, Ld, at)
    rot = data.apply_galois(ct, g)
    switched = ks.divide_and_add(ks.key_products(orc, ks.lift(rot[1], p.moduli, Ld, alpha), key[0]), rot, p.moduli, Ld, at)
    for (comp, k), words in switched.items():
        assert got[comp, k] == [(w + int(ct[comp, j, k])) % int(p.moduli[j]) for j, w in enumerate(words)], (comp, k)
