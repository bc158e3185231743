"""The counter-based generator behind seed= of sample_boltzmann, relax_samples, exchange_clusters, temper_samples and anneal_population
(tn_uniforms, csrc/rng.hip).

Every uniform number is a pure function U(seed, stream, i) of three unsigned 64-bit numbers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw
2011) on the counter (b lo32, b hi32, stream lo32, stream hi32), b = i >> 1, with the key (seed lo32, seed hi32) gives four 32-bit words
x; with h = i & 1 and v = x[2h] + 2^32 x[2h+1], U = (v >> 11) 2^-53 in [0, 1 - 2^-53].  The stream says what a number is for:
stream_id(kind, row) = kind 2^56 + row with the kinds below, and i is the last index of the array -- the sample, except for the draw
of a fresh population, where the sample is the row.  A number therefore depends on its logical position alone: not on the grid, not
on chunk, not on how rounds or steps are cut into calls, and not on how many samples there are.

The host part (uniforms_host: the same function in vectorised numpy; the pairings; the seed rule) runs without a GPU: it decides
everything a call refuses, and every pairing, before any device work."""
import operator

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                            # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                            # key increments
TWO64 = 1 << 64
ROW_LIMIT = 1 << 56

# kind: array (logical shape) -- row = the C-order index over all dimensions but the last, i = the last index
WALK = 1                 # sample_boltzmann walk (ncell, M)
RELAX_SWEEP = 2          # relax_samples sweep (sweeps, ncell, M)
EXCHANGE_SEED = 3        # exchange_clusters seeds (rounds, P)
EXCHANGE_PAIRING = 4     # exchange_clusters pairing keys (rounds, M)
TEMPER_SWEEP = 5         # temper_samples sweep (rounds, sweeps, ncell, M)
TEMPER_CLUSTER = 6       # temper_samples cluster (rounds, Tc, Pc)
TEMPER_SWAP = 7          # temper_samples swap (rounds, R, T - 1)
TEMPER_PAIRING = 8       # temper_samples pairing keys (rounds, R)
ANNEAL_INIT = 9          # anneal_population init (M, ncell)
ANNEAL_RESAMPLE = 10     # anneal_population resample (K - 1,): row 0
ANNEAL_SWEEP = 11        # anneal_population sweep (K - 1, sweeps, ncell, M)
RELAX_LINE = 12          # relax_lines sweep (sweeps, passes, ncell, M)


def check_seed(seed):
    """None, or an integer in [0, 2^64) (returned as int); a bool or anything else: ValueError."""
    if seed is None:
        return None
    if isinstance(seed, (bool, np.bool_)):
        raise ValueError('seed must be None or an integer in [0, 2^64) (got a bool)')
    try:
        s = operator.index(seed)
    except TypeError:
        raise ValueError('seed must be None or an integer in [0, 2^64) (got %s)' % type(seed).__name__)
    if not 0 <= s < TWO64:
        raise ValueError('seed must lie in [0, 2^64) (got %d)' % s)
    return s


def check_seed_alone(seed, uniforms):
    """check_seed, and a ValueError when a seed comes with uniforms: the numbers have one source."""
    seed = check_seed(seed)
    if seed is not None and uniforms is not None:
        raise ValueError('seed and uniforms exclude each other: give one source of the uniform numbers')
    return seed


def stream_id(kind, row):
    """kind 2^56 + row; kind in [0, 256), row in [0, 2^56): ValueError otherwise."""
    kind, row = operator.index(kind), operator.index(row)
    if not 0 <= kind < 256:
        raise ValueError('kind must lie in [0, 256)')
    if not 0 <= row < ROW_LIMIT:
        raise ValueError('row must lie in [0, 2^56) (got %d)' % row)
    return kind * ROW_LIMIT + row


def philox4x32_10(counter, key):
    """Philox4x32-10 in numpy: counter = four and key = two uint32 arrays of one shape (or scalars); returns the four output words."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k = [np.asarray(x, dtype=np.uint64) for x in key]
    lo32, m0, m1 = np.uint64(0xFFFFFFFF), np.uint64(M0), np.uint64(M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                       # 32 x 32 -> 64 bits, exact
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & lo32, (p0 >> s32) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(W0)) & lo32, (k[1] + np.uint64(W1)) & lo32]
    return [x.astype(np.uint32) for x in c]


def uniforms_host(seed, stream, first, n):
    """(n,) float64: U(seed, stream, first + c) for c < n, the numbers tn_uniforms writes into one row.  seed, stream, first in
    [0, 2^64), first + n <= 2^64: ValueError otherwise."""
    seed, stream, first, n = (operator.index(v) for v in (seed, stream, first, n))
    for name, v in (('seed', seed), ('stream', stream), ('first', first)):
        if not 0 <= v < TWO64:
            raise ValueError('%s must lie in [0, 2^64)' % name)
    if n < 0 or first + n > TWO64:
        raise ValueError('n must not be negative and first + n must not pass 2^64')
    i = np.uint64(first) + np.arange(n, dtype=np.uint64)
    b = i >> np.uint64(1)
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    full = np.full(n, 0, dtype=np.uint64)
    x = philox4x32_10((b & lo32, b >> s32, full + np.uint64(stream & 0xFFFFFFFF), full + np.uint64(stream >> 32)),
                      (full + np.uint64(seed & 0xFFFFFFFF), full + np.uint64(seed >> 32)))
    odd = (i & np.uint64(1)).astype(bool)
    v = np.where(odd, x[2], x[0]).astype(np.uint64) | (np.where(odd, x[3], x[1]).astype(np.uint64) << s32)
    return (v >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def rows_host(seed, kind, row0, rows, first, cols):
    """(rows, cols) float64: the numbers of the rows row0 .. row0 + rows - 1 of a kind, columns first .. first + cols - 1 (host)."""
    if rows > 0:
        stream_id(kind, row0 + rows - 1)
    out = np.empty((rows, cols))
    for r in range(rows):
        out[r] = uniforms_host(seed, stream_id(kind, row0 + r), first, cols)
    return out


def pairs_from_keys(keys):
    """The pairing of one round from its keys (n,): perm = the stable ascending argsort, pairs = perm[:2 P].reshape(P, 2), P = n // 2."""
    keys = np.asarray(keys)
    P = keys.size // 2
    return np.argsort(keys, kind='stable')[:2 * P].reshape(P, 2)


def draw_pairs(seed, kind, rounds, n):
    """(rounds, n // 2, 2) int32: the pairings of the rounds 0 .. rounds - 1 over n rows from the pairing keys of `kind` (host)."""
    P = n // 2
    keys = rows_host(seed, kind, 0, rounds, 0, n)
    return np.array([pairs_from_keys(keys[r]) for r in range(rounds)], dtype=np.int32).reshape(rounds, P, 2)


def fill(seed, kind, row0, shape, first=0, dev=None):
    """A device tensor of `shape` with the numbers of a kind: its rows -- the C-order index over all dimensions but the last -- are the
    rows row0 .. of the kind, its last dimension the indices first ..  One tn_uniforms."""
    import torch
    from . import ops
    shape = tuple(int(s) for s in shape)
    cols = shape[-1]
    rows = int(np.prod(shape[:-1], dtype=np.int64)) if len(shape) > 1 else 1
    if rows > 0:
        stream_id(kind, row0 + rows - 1)
    out = torch.empty(shape, dtype=torch.float64, device=dev if dev is not None else torch.device('cuda', torch.cuda.current_device()))
    if rows > 0 and cols > 0:
        ops.uniforms(seed, stream_id(kind, row0), first, rows, cols, out=out.view(rows, cols))
    return out
