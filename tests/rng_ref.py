"""Scalar restatement of the library's counter-based generator in Python integers, written from the definition and
importing nothing from the package: Philox4x32-10, the number U(seed, stream, i), the stream ids, the pairing rule, and a builder for
every array of the kind table in the layout the public calls take as uniforms= (and pairs=)."""
from functools import lru_cache

import numpy as np

MASK32 = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85

# the published known answers: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
# seed, stream, the raw block at b = 0, U(., ., 0), U(., ., 1)
KNOWN = (20260004, 7, (3175488781, 752980204, 1197805648, 855737833), float.fromhex('0x1.670c8765ea30cp-3'), float.fromhex('0x1.980c2f4a3b288p-3'))


def same_bits(a, b):
    """Bit-for-bit equality of two numpy arrays."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


@lru_cache(maxsize=1 << 16)
def block(seed, stream, b):
    return philox((b & MASK32, b >> 32, stream & MASK32, stream >> 32), (seed & MASK32, seed >> 32))


def U(seed, stream, i):
    assert 0 <= seed < 1 << 64 and 0 <= stream < 1 << 64 and 0 <= i < 1 << 64
    x = block(seed, stream, i >> 1)
    h = i & 1
    v = x[2 * h] + (x[2 * h + 1] << 32)
    return float(v >> 11) * 2.0 ** -53


def stream_id(kind, row):
    assert 0 <= row < 1 << 56
    return (kind << 56) + row


def fill(seed, stream0, first, rows, cols):
    """(rows, cols): what tn_uniforms writes."""
    return np.array([[U(seed, stream0 + r, first + c) for c in range(cols)] for r in range(rows)], dtype=np.float64).reshape(rows, cols)


def pairs_from_keys(keys):
    """perm = the stable ascending argsort, pairs = perm[:2 P].reshape(P, 2)."""
    n = len(keys)
    perm = sorted(range(n), key=lambda m: (keys[m], m))
    P = n // 2
    return np.array(perm[:2 * P], dtype=np.int64).reshape(P, 2)


# ---------------------------------------------------------------------------------------------- the arrays of the kind table
def walk(seed, ncell, M):                                                # kind 1: sample_boltzmann (ncell, M)
    return np.array([[U(seed, stream_id(1, k), m) for m in range(M)] for k in range(ncell)]).reshape(ncell, M)


def relax_sweep(seed, sweeps, ncell, M):                                 # kind 2: relax_samples (sweeps, ncell, M)
    return np.array([[[U(seed, stream_id(2, j * ncell + k), m) for m in range(M)] for k in range(ncell)] for j in range(sweeps)]).reshape(sweeps, ncell, M)


def exchange_seeds(seed, rounds, P):                                     # kind 3: exchange_clusters (rounds, P)
    return np.array([[U(seed, stream_id(3, r), p) for p in range(P)] for r in range(rounds)]).reshape(rounds, P)


def exchange_pairs(seed, rounds, M):                                     # kind 4: pairing keys (rounds, M) -> (rounds, M // 2, 2)
    return np.array([pairs_from_keys([U(seed, stream_id(4, r), m) for m in range(M)]) for r in range(rounds)], dtype=np.int64).reshape(rounds, M // 2, 2)


def temper_uniforms(seed, rounds, sweeps, ncell, M, T, Tc, Pc):          # kinds 5, 6, 7
    R = M // T
    sw = np.array([[[[U(seed, stream_id(5, (r * sweeps + j) * ncell + k), m) for m in range(M)] for k in range(ncell)] for j in range(sweeps)]
                   for r in range(rounds)]).reshape(rounds, sweeps, ncell, M)
    cl = np.array([[[U(seed, stream_id(6, r * Tc + t), p) for p in range(Pc)] for t in range(Tc)] for r in range(rounds)]).reshape(rounds, Tc, Pc)
    sp = np.array([[[U(seed, stream_id(7, r * R + c), t) for t in range(T - 1)] for c in range(R)] for r in range(rounds)]).reshape(rounds, R, T - 1)
    return {'sweep': sw, 'cluster': cl, 'swap': sp}


def temper_pairs(seed, rounds, R):                                       # kind 8: pairing keys (rounds, R)
    return np.array([pairs_from_keys([U(seed, stream_id(8, r), c) for c in range(R)]) for r in range(rounds)], dtype=np.int64).reshape(rounds, R // 2, 2)


def anneal_uniforms(seed, K, sweeps, ncell, M, fresh):                   # kinds 9, 10, 11
    u = {'resample': np.array([U(seed, stream_id(10, 0), s) for s in range(K - 1)]).reshape(K - 1),
         'sweep': np.array([[[[U(seed, stream_id(11, (s * sweeps + j) * ncell + k), m) for m in range(M)] for k in range(ncell)] for j in range(sweeps)]
                            for s in range(K - 1)]).reshape(K - 1, sweeps, ncell, M)}
    if fresh:
        u['init'] = np.array([[U(seed, stream_id(9, m), k) for k in range(ncell)] for m in range(M)]).reshape(M, ncell)
    return u
