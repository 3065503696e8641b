"""shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import hashlib

import numpy as np


def limbs(hexlist):
    return np.array([int(h, 16) for h in hexlist], dtype=np.uint64)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def sha_inplace(a):
    """sha(a) without the copy tobytes() makes (vectors of several GiB)"""
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return hashlib.sha256(a.reshape(-1).view(np.uint8).data).hexdigest()


def noncanonical(coeffs, fr_modulus):
    """+r on every third element: inputs in [0, 2r) as the prover produces."""
    out = coeffs.copy()
    mod = np.array([(fr_modulus >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    idx = np.arange(0, out.shape[0], 3)
    carry = np.zeros(idx.shape[0], dtype=np.uint64)
    for l in range(4):
        a = out[idx, l]
        s = a + mod[l]
        c1 = (s < a).astype(np.uint64)
        s2 = s + carry
        c2 = (s2 < s).astype(np.uint64)
        out[idx, l] = s2
        carry = c1 + c2
    return out


def _mod_limbs(fr_modulus):
    return [np.uint64((fr_modulus >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4)]


def lift_max(a, fr_modulus, chunk=1 << 20):
    """IN PLACE: every element x of the (n, 4) array becomes its largest representative below 2^256, x + k r with k as large as fits:
    k = #{j in 1..5 : x < 2^256 - j r} (2^256 / r < 6; any x in [0, 2^256) is accepted).  The residues are unchanged; the values are the
    largest a transform can be handed.  Returns a."""
    top = 1 << 256
    thresholds = [_mod_limbs(top - j * fr_modulus) for j in range(1, 6)]
    multiples = np.array([_mod_limbs(j * fr_modulus) for j in range(6)], dtype=np.uint64)
    for lo in range(0, a.shape[0], chunk):
        blk = a[lo:lo + chunk]
        x = [np.ascontiguousarray(blk[:, l]) for l in range(4)]
        k = np.zeros(blk.shape[0], dtype=np.intp)
        for t in thresholds:
            lt = x[0] < t[0]
            for l in range(1, 4):
                lt = (x[l] < t[l]) | ((x[l] == t[l]) & lt)
            k += lt
        add = multiples[k]
        carry = np.zeros(blk.shape[0], dtype=np.uint64)
        for l in range(4):
            s = x[l] + add[:, l]
            c1 = s < x[l]
            s2 = s + carry
            blk[:, l] = s2
            carry = (c1 | (s2 < s)).astype(np.uint64)
    return a


def lift_extremes(fr_modulus):
    """raw values at the edges of the input range: 0, r - 1, r, 2r, 5r (the largest multiple of r below 2^256), 2^256 - 1"""
    return [0, fr_modulus - 1, fr_modulus, 2 * fr_modulus, 5 * fr_modulus, (1 << 256) - 1]


def extreme_positions(n, count):
    """where a vector of n elements holds the `count` raw extremes (for n < count later ones overwrite earlier ones)"""
    return [(i * n) // count for i in range(count)]


SCALAR_SEED = 0x9E3779B97F4A7C15
SRS_SEED = 0x5EED0F5EC2E7C0DE
NTT_SEED = 0x0123456789ABCDEF
CONST_SEED = 0x00C0FFEE00C0FFEE
